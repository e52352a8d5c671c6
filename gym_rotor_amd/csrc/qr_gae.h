// qr_gae.h — part of the gfx950 quadrotor step library (included by quadrotor_kernels.hip, after qr_episode.h).
// PPO's advantages with the done flag the reference stores (qr_gae_rule): main.py:169-173 overwrites done_n at the episode time limit
// with "solved and not crashed" before main.py:176-177 stores it, and ppo.py:134-146 reads that flag twice — in the TD error's
// (1 - done) and in the (1 - done) that cuts the lambda-recursion.  Three kernels behind one C call:
//   gae_rule_kernel       gae_kernel's reverse scan (qr_aux.h) over the EFFECTIVE flag, with per-agent float64 partial sums
//   gae_fold_kernel       the partial vectors folded in workgroup-index order into stats[n_agents][3] (sum, sum of squares, count)
//   gae_normalize_kernel  (adv - mean) / (std + eps), ppo.py:146 with torch's unbiased std, elementwise
//
// The scan has gae_kernel's shape: 64-lane workgroups, one lane per (env, agent) column j = n * NAG + k, serial in t backwards, the
// loads of kGaeU steps — the truncated byte among them — issued ahead of the recurrence.  The terminal-observation words are read
// inside the recurrence, on truncated rows only: a dependent round trip for the block that holds such a row, none elsewhere.
// The float32 recurrence is gae_kernel's text, expression for expression, so that the result equals qr_gae run on done_eff bit for bit.
// No existing kernel is touched.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "quadrotor_hip.h"
#include "qr_replay.h"

namespace qr {

constexpr int kGaeU = 8;   // steps whose loads are in flight per lane (gae_kernel's kU)
constexpr int kGaeNormGrid = 2048;   // workgroups of the normalise pass at the most (it strides over the rest)

struct GaeRuleArgs {
  const float* reward; const uint8_t* done; const uint8_t* truncated;
  const float* obs0; const float* obs1;   // the transitions' obs_next rows (read where truncated is set)
  const float* value; const float* next_value;
  float* advantage; float* td_target; uint8_t* done_eff;
  double* partials;                        // [grid][NAG][2], or null
  int64_t n;                               // envs
  int32_t T, d0, d1, rule;
  float gamma, lam;
  double x_lim, pos_tol, rot_tol;
};

template <int NAG>
__global__ __launch_bounds__(64) void gae_rule_kernel(const GaeRuleArgs g) {
  constexpr int kU = kGaeU;
  const int64_t j = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const int64_t N = g.n;
  const int64_t M = N * NAG;
  const bool active = j < M;
  const int k = NAG == 2 ? (int)(threadIdx.x & 1u) : 0;   // (64 is even: the agent of a column is its lane's parity)
  const int64_t n = NAG == 2 ? (j >> 1) : j;
  float adv = 0.0f;
  double s1 = 0.0, s2 = 0.0;
  if (active) {
    float vnext = g.next_value ? 0.0f : g.value[(int64_t)g.T * M + j];  // bootstrap row
    for (int t0 = g.T; t0 > 0; t0 -= kU) {
      const int nb = t0 < kU ? t0 : kU;
      float r[kU], v[kU], vn[kU];
      uint8_t d[kU], tr[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        if (u < nb) {
          const int64_t idx = (int64_t)(t0 - 1 - u) * M + j;
          r[u] = g.reward[idx]; d[u] = g.done[idx]; v[u] = g.value[idx];
          vn[u] = g.next_value ? g.next_value[idx] : 0.0f;
          tr[u] = g.rule ? g.truncated[(int64_t)(t0 - 1 - u) * N + n] : (uint8_t)0;
        }
      }
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        if (u < nb) {
          const int64_t idx = (int64_t)(t0 - 1 - u) * M + j;
          uint8_t de = d[u];
          if (tr[u] != 0) {   // (the replay rule's expressions, qr_replay_walk.h: double arithmetic on the float32 words)
            const int64_t row = (int64_t)(t0 - 1 - u) * N + n;
            bool solved;
            if (k == 0) {
              const float* s0 = g.obs0 + row * g.d0;
              solved = fabs((double)s0[0] * g.x_lim) <= g.pos_tol;
              solved = solved & (fabs((double)s0[1] * g.x_lim) <= g.pos_tol);
              solved = solved & (fabs((double)s0[2] * g.x_lim) <= g.pos_tol);
            } else {
              solved = fabs((double)g.obs1[row * g.d1] * kReplayPi) <= g.rot_tol;
            }
            de = (solved & (r[u] != -1.0f)) ? (uint8_t)1 : (uint8_t)0;
          }
          const float nd = de ? 0.0f : 1.0f;
          const float vnx = g.next_value ? vn[u] : vnext;
          const float delta = r[u] + g.gamma * vnx * nd - v[u];
          adv = delta + g.gamma * nd * g.lam * adv;
          g.advantage[idx] = adv;
          g.td_target[idx] = adv + v[u];
          if (g.done_eff) g.done_eff[idx] = de;
          s1 += (double)adv; s2 += (double)adv * (double)adv;
          vnext = v[u];
        }
      }
    }
  }
  if (g.partials) {   // a fixed shuffle tree over the lanes of equal k (lane l takes lane l + off), one vector per workgroup, no atomics
#pragma unroll
    for (int off = 32; off >= NAG; off >>= 1) { s1 += __shfl_down(s1, off); s2 += __shfl_down(s2, off); }
    if (threadIdx.x < NAG) {
      double* p = g.partials + ((int64_t)blockIdx.x * NAG + threadIdx.x) * 2;
      p[0] = s1; p[1] = s2;
    }
  }
}

struct GaeFoldArgs {
  const double* partials;   // [n_parts][n_fields]
  double* stats;            // [n_agents][3]
  int32_t n_parts, n_fields;   // n_fields = 2 * n_agents
  double count;             // T * N
};

// One workgroup.  Thread t folds, per field, the vectors t, t + 256, ... in that order, then a tree over the 256 slices
// (episode_reduce_kernel's order): the result is a function of the vectors' index order alone.
__global__ __launch_bounds__(256) void gae_fold_kernel(const GaeFoldArgs o) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  for (int f = 0; f < o.n_fields; ++f) {
    double mine = 0.0;
    for (int p = t; p < o.n_parts; p += 256) mine += o.partials[(int64_t)p * o.n_fields + f];
    __syncthreads();
    red[t] = mine;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
      if (t < w) red[t] += red[t + w];
      __syncthreads();
    }
    if (t == 0) o.stats[(f >> 1) * 3 + (f & 1)] = red[0];
  }
  if (t < (o.n_fields >> 1)) o.stats[t * 3 + 2] = o.count;
}

struct GaeNormArgs {
  const float* advantage; const double* stats; float* out;
  int64_t count;            // T * N * n_agents elements
  double eps;
};

// Grid-stride and elementwise.  VEC: both pointers are 16-byte aligned — four elements per lane and access (4 is a multiple of NAG, so
// element c of a quad belongs to agent c % NAG); the count's remainder goes to the first lanes of workgroup 0.  mean and std are
// RolloutStorage.normalize's expressions on the same stats, in double (the build contracts n * mean * mean into the subtraction, which
// moves the variance by a rounding error of that product: far inside the one float32 rounding the result gets).
template <int NAG, bool VEC>
__global__ __launch_bounds__(256) void gae_normalize_kernel(const GaeNormArgs a) {
  double mean[NAG], den[NAG];
#pragma unroll
  for (int k = 0; k < NAG; ++k) {
    const double s1 = a.stats[k * 3], s2 = a.stats[k * 3 + 1], n = a.stats[k * 3 + 2];
    mean[k] = s1 / n;
    const double var = (s2 - n * mean[k] * mean[k]) / (n - 1.0);
    den[k] = sqrt(var > 0.0 ? var : 0.0) + a.eps;
  }
  const double mean0 = mean[0], den0 = den[0], mean1 = mean[NAG - 1], den1 = den[NAG - 1];   // (one agent: both are agent 0's)
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * 256;
  if constexpr (VEC) {
    const int64_t quads = a.count >> 2;
    for (int64_t q = tid; q < quads; q += stride) {
      const float4 x = reinterpret_cast<const float4*>(a.advantage)[q];
      float4 y;
      y.x = (float)(((double)x.x - mean0) / den0);
      y.y = (float)(((double)x.y - mean1) / den1);
      y.z = (float)(((double)x.z - mean0) / den0);
      y.w = (float)(((double)x.w - mean1) / den1);
      reinterpret_cast<float4*>(a.out)[q] = y;
    }
    const int64_t e = (quads << 2) + tid;
    if (e < a.count) {   // (at most three elements)
      const bool odd = NAG == 2 && (e & 1);
      a.out[e] = (float)(((double)a.advantage[e] - (odd ? mean1 : mean0)) / (odd ? den1 : den0));
    }
  } else {
    for (int64_t e = tid; e < a.count; e += stride) {
      const bool odd = NAG == 2 && (e & 1);
      a.out[e] = (float)(((double)a.advantage[e] - (odd ? mean1 : mean0)) / (odd ? den1 : den0));
    }
  }
}

}  // namespace qr
