// qr_episode.h — part of the gfx950 quadrotor step library (included by quadrotor_kernels.hip, after qr_replay.h).
// The training curve of the reference's loop (main.py:132-137, 180, 212-235) from the rows a collected horizon has already written
// (qr_episode_scan): which episodes finished inside the T x N transitions, how long they were, what they returned, how they ended and
// how close to the goal — episode_scan_kernel — and their statistics, for this launch and accumulated — episode_reduce_kernel.
//
// The scan has gae_kernel's shape (qr_aux.h): one lane per env, serial in t (here forwards), the loads of kEpU steps issued ahead of
// the recurrence, so that a wave keeps kEpU rows in flight instead of paying one memory round trip per step.  The terminal observation
// is read only on the rows where an episode ended.  No existing kernel is touched: the scan reads what the step kernels stored.
//
// Deliberate deviation, the one QrEvalOut.episode_return documents: the reference rounds its running return to 4 decimals at every
// step (main.py:180: float('{:.4f}'.format(...))); here the float32 rewards are summed in float64 and not rounded, so a return differs
// from the reference's by at most 0.5e-4 per step of the episode (tests/test_episode_host.py holds that bound).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "quadrotor_hip.h"
#include "qr_replay.h"

namespace qr {

constexpr int kEpU = 8;                    // steps whose loads are in flight per lane
constexpr int kEpK = QR_EP_FIELDS;         // fields of a partial vector, of `last` and (plus steps_seen) of `total`

struct EpisodeScanArgs {
  const float* reward; const uint8_t* done; const uint8_t* truncated;
  const float* fin0; const float* fin1;    // terminal observation rows, or null
  double* run_return; int32_t* run_length; // the carries
  double* ep_return; int32_t* ep_length; uint8_t* ep_flags; float* ep_final_error;   // dense rows, each may be null
  double* partials;                        // [grid][kEpK]
  int64_t n;
  int32_t T, d0, d1, record;
  double x_lim, pos_tol, rot_tol;
};

// how field k folds: 0 a sum (counts are sums), 1 a minimum, 2 a maximum
__host__ __device__ constexpr int ep_fold_kind(int k) {
  return (k == QR_EP_RETURN_MIN || k == QR_EP_RETURN_MIN + 1) ? 1 : (k == QR_EP_RETURN_MAX || k == QR_EP_RETURN_MAX + 1 || k == QR_EP_LENGTH_MAX) ? 2 : 0;
}
// the field of a vector over no episodes
__host__ __device__ constexpr double ep_empty(int k) {
  return (k == QR_EP_RETURN_MIN || k == QR_EP_RETURN_MIN + 1) ? __builtin_huge_val()
       : (k == QR_EP_RETURN_MAX || k == QR_EP_RETURN_MAX + 1) ? -__builtin_huge_val() : 0.0;
}
__device__ __forceinline__ double ep_fold(int kind, double a, double b) { return kind == 0 ? a + b : kind == 1 ? (b < a ? b : a) : (b > a ? b : a); }

template <int NAG>
__global__ __launch_bounds__(64) void episode_scan_kernel(const EpisodeScanArgs a) {
  const int64_t N = a.n;
  const int64_t n = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const bool active = n < N;
  double st[kEpK];
#pragma unroll
  for (int k = 0; k < kEpK; ++k) st[k] = ep_empty(k);
  if (active) {
    double ret[NAG];
#pragma unroll
    for (int g = 0; g < NAG; ++g) ret[g] = a.run_return[n * NAG + g];
    int32_t len = a.run_length[n];
    for (int t0 = 0; t0 < a.T; t0 += kEpU) {
      const int nb = a.T - t0 < kEpU ? a.T - t0 : kEpU;
      float r[kEpU][NAG];
      uint8_t d[kEpU][NAG], tr[kEpU];
#pragma unroll
      for (int u = 0; u < kEpU; ++u) {
        if (u < nb) {
          const int64_t row = (int64_t)(t0 + u) * N + n;
          if constexpr (NAG == 2) {
            const float2 v = reinterpret_cast<const float2*>(a.reward)[row];
            r[u][0] = v.x; r[u][1] = v.y;
            d[u][0] = a.done[row * 2]; d[u][1] = a.done[row * 2 + 1];
          } else {
            r[u][0] = a.reward[row];
            d[u][0] = a.done[row];
          }
          tr[u] = a.truncated[row];
        }
      }
#pragma unroll
      for (int u = 0; u < kEpU; ++u) {
        if (u < nb) {
          const int64_t row = (int64_t)(t0 + u) * N + n;
#pragma unroll
          for (int g = 0; g < NAG; ++g) ret[g] += (double)r[u][g];
          len += 1;
          const bool limit = tr[u] != 0;
          bool ended = limit;
#pragma unroll
          for (int g = 0; g < NAG; ++g) ended = ended | (d[u][g] != 0);
          double out_ret[NAG];
#pragma unroll
          for (int g = 0; g < NAG; ++g) out_ret[g] = 0.0;
          int32_t out_len = 0;
          uint32_t flags = 0;
          float fe[4] = {0.0f, 0.0f, 0.0f, 0.0f};
          if (ended) {
            double ex[3] = {0.0, 0.0, 0.0}, eb1 = 0.0;
            bool solved[2] = {false, false};
            if (a.fin0) {   // (the replay rule's expressions, qr_replay_walk.h: double arithmetic on the float32 words)
              const float* s0 = a.fin0 + row * a.d0;
#pragma unroll
              for (int c = 0; c < 3; ++c) ex[c] = (double)s0[c] * a.x_lim;
              solved[0] = (fabs(ex[0]) <= a.pos_tol) & (fabs(ex[1]) <= a.pos_tol) & (fabs(ex[2]) <= a.pos_tol) & (r[u][0] != -1.0f);
              if constexpr (NAG == 2) {
                eb1 = (double)a.fin1[row * a.d1] * kReplayPi;
                solved[1] = (fabs(eb1) <= a.rot_tol) & (r[u][1] != -1.0f);
              }
            }
#pragma unroll
            for (int g = 0; g < NAG; ++g) {
              flags |= d[u][g] != 0 ? (1u << g) : 0u;
              flags |= (limit & solved[g]) ? (QR_EP_FLAG_SOLVED0 << g) : 0u;
            }
            flags |= limit ? QR_EP_FLAG_TRUNCATED : 0u;
#pragma unroll
            for (int c = 0; c < 3; ++c) fe[c] = (float)ex[c];
            fe[3] = (float)eb1;
            out_len = len;
            if (a.record) {
              st[QR_EP_COUNT] += 1.0;
#pragma unroll
              for (int g = 0; g < NAG; ++g) {
                st[QR_EP_RETURN_SUM + g] += ret[g];
                st[QR_EP_RETURN_SQ + g] += ret[g] * ret[g];
                st[QR_EP_RETURN_MIN + g] = ep_fold(1, st[QR_EP_RETURN_MIN + g], ret[g]);
                st[QR_EP_RETURN_MAX + g] = ep_fold(2, st[QR_EP_RETURN_MAX + g], ret[g]);
                st[QR_EP_DONE + g] += d[u][g] != 0 ? 1.0 : 0.0;
                st[QR_EP_SOLVED + g] += (limit & solved[g]) ? 1.0 : 0.0;
              }
              st[QR_EP_LENGTH_SUM] += (double)len;
              st[QR_EP_LENGTH_MAX] = ep_fold(2, st[QR_EP_LENGTH_MAX], (double)len);
              st[QR_EP_TRUNCATED] += limit ? 1.0 : 0.0;
              const double e01 = fabs(ex[0]) > fabs(ex[1]) ? fabs(ex[0]) : fabs(ex[1]);
              st[QR_EP_EX_SUM] += e01 > fabs(ex[2]) ? e01 : fabs(ex[2]);
              st[QR_EP_EB1_SUM] += fabs(eb1);
            }
#pragma unroll
            for (int g = 0; g < NAG; ++g) { out_ret[g] = ret[g]; ret[g] = 0.0; }
            len = 0;
          }
          if (a.ep_return) {
#pragma unroll
            for (int g = 0; g < NAG; ++g) a.ep_return[row * NAG + g] = out_ret[g];
          }
          if (a.ep_length) a.ep_length[row] = out_len;
          if (a.ep_flags) a.ep_flags[row] = (uint8_t)flags;
          if (a.ep_final_error) reinterpret_cast<float4*>(a.ep_final_error)[row] = make_float4(fe[0], fe[1], fe[2], fe[3]);
        }
      }
    }
#pragma unroll
    for (int g = 0; g < NAG; ++g) a.run_return[n * NAG + g] = ret[g];
    a.run_length[n] = len;
  }
  // the wave's vector: a fixed shuffle tree (lane l takes lane l + off), one vector per workgroup, no atomics
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int k = 0; k < kEpK; ++k) st[k] = ep_fold(ep_fold_kind(k), st[k], __shfl_down(st[k], off));
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < kEpK; ++k) a.partials[(int64_t)blockIdx.x * kEpK + k] = st[k];
  }
}

struct EpisodeReduceArgs {
  const double* partials;   // [n_parts][kEpK]
  double* last;             // [kEpK]
  double* total;            // [kEpK + 1]
  int32_t n_parts, T, record;
};

// One workgroup.  Thread t folds, per field, the vectors t, t + 256, ... in that order, then a tree over the 256 slices
// (ppo_critic_reduce_kernel's order): the result is a function of the vectors' index order alone.
__global__ __launch_bounds__(256) void episode_reduce_kernel(const EpisodeReduceArgs o) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  for (int k = 0; k < kEpK; ++k) {
    const int kind = ep_fold_kind(k);
    double mine = ep_empty(k);
    if (o.record)
      for (int p = t; p < o.n_parts; p += 256) mine = ep_fold(kind, mine, o.partials[(int64_t)p * kEpK + k]);
    __syncthreads();
    red[t] = mine;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
      if (t < w) red[t] = ep_fold(kind, red[t], red[t + w]);
      __syncthreads();
    }
    if (t == 0) {
      o.last[k] = red[0];
      if (o.record) o.total[k] = ep_fold(kind, o.total[k], red[0]);
    }
  }
  if (t == 0) o.total[QR_EP_STEPS_SEEN] += (double)o.T;
}

}  // namespace qr
