// qr_td3_actor.h — part of the gfx950 quadrotor step library (included by quadrotor_kernels.hip only, after qr_td3.h).
// The actor half of one TD3 minibatch update (TD3.train, algos/td3/td3.py:177-211, the non-CTDE branch, plus
// algos/policy_regularization.py):
//   dpg_actor_kernel + dpg_reduce_kernel (qr_dpg_actor_grad)   -mean Q1(s, pi(s)) with the three smoothness terms, and its gradients
//                                                               for MLP_Actor_TD3's six tensors
//   ctde_dpg_actor_kernel + dpg_reduce_kernel (qr_ctde_dpg_actor_grad)   the same for agent k of two under ONE centralized (CTDE) critic
//                                                               (td3.py:180-196): the same walk (dpg_walk) in its two-agent form
//   soft_update_kernel (qr_soft_update)                         target = tau param + (1 - tau) target for up to 24 tensors
// The pieces are shared: the actor's passes are PpoNet's (qr_ppo.h: forward, backward, the MFMA weight gradients, emit), Q1's forward
// pass and the product W2^T dz2 are qr_mlp_grad.h's pieces with qr_td3.h's TwinQL1, the reduction is reduce16_entries /
// block_sum_column, and the host launcher is ppo_actor_kernel's (actor_grad_launch).  New: the contraction
// dQ/da = fc1_w[:, D..D+A)^T dz1, and the glue.  The tile walk — prologue, gather, smoothness block, epilogue — IS a second copy of
// ppo_actor_kernel's: with the loss phase below as a hook of a shared walk this kernel takes 8 more AGPRs, so a fix
// to either walk has to be made in both.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "quadrotor_hip.h"
#include "qr_ppo.h"
#include "qr_td3.h"

namespace qr {

struct DpgArgs {
  ActorW w;                          // pi: log_std points at readable floats (PpoNet::fill copies them; nothing here reads the copy)
  MlpNetW q;                         // Q1
  const float *obs, *obs_next;       // [>= rows][D]; obs_next is read with lam_T != 0 only
  const int64_t* index;              // [B] or NULL (rows 0..B-1)
  const float *noise, *nominal;      // [D], [A]
  double* partials;                  // [grid][NP]
  int64_t B, rows;
  int32_t hidden;                    // of the critic
  float max_action;
  float lam_T, lam_S, lam_M;         // only their being zero is read here (wave-uniform branches)
  float inv_b, c_T, c_S, c_M;        // 1 / B and 2 lam / (B A): the per-row factors of the gradient
};

// The centralized (CTDE) form for agent k of two (qr_ctde_dpg_actor_grad): DpgArgs' members are agent k's (w = pi_k, obs / obs_next /
// noise / nominal its own), q = Q1 of the centralized critic whose row is [obs_0 | obs_1 | a_0 | a_1].
struct CtdeDpgArgs : DpgArgs {
  ActorW other;                      // pi_{1-k}, forward only (log_std and the log_std head NULL); read when action_other is NULL
  const float* obs_other;            // [>= rows][od_other]
  const float* action_other;         // [B][ad_other] by minibatch position, used as it is, or NULL: pi_{1-k}'s clamped output
  int32_t od_other, ad_other;        // the other agent's widths
  int32_t col_own, col_other;        // first column of each agent's observation in the critic's row
  int32_t acol_own, acol_other;      // first column of each agent's action: D + off_k, D + off_{1-k}
  int32_t in_dim;                    // the row's width, <= 28
};

// One workgroup's partial vector: PpoLayout's six weight and bias tensors, then the five sums of `stats`:
// 0 Q1, 1 components of pi(obs) outside +-max_action, 2 / 3 / 4 the squared differences of the temporal, spatial and magnitude terms
template <int D, int H, int A>
struct DpgLayout {
  static constexpr int O_ST = PpoLayout<D, H, A>::O_LS, NS = 5, NP = O_ST + NS;
};
constexpr int kDpgQ = 5;  // row stride of the tile that carries dQ/da (4 columns) and Q back to the rows' lanes; odd

// Q1 and dQ1/da of one half tile (32 rows of qs = [obs | a | 0..], stride kMgX) in mlp_grad_half's lane map: forward on the matrix
// cores, dz2 = fc3_w (t2 > 0), dz1 = (W2^T dz2)(t1 > 0) — the same MFMA loop as layer 2 with the transposed operands —, then the
// contraction over the hidden units  dQ/da[row][j] = sum_u fc1_w[u][D + j] dz1[row][u]:  a lane's 16 units on the VALU (wa: the A
// action columns of fc1_w as [64 units][4], zero past H and A, read as broadcasts), then the sum over the four lanes of a row.
// fc2_w is resident (a2); its transpose's operands come from LDS (w2t: entry e = (hi, kb, r) of lane l at [64 e + l], one dword per
// lane) and live only here: resident as in twinq_kernel they would not leave the actor's passes their registers.
template <int A>
__device__ __forceinline__ void dpg_q1_half(const float (&a2)[4][4][4], const float* w2t, const float* qh, const float* w1, const float* sv,
                                            const float* wa0, float* dq, float bias3, int lane) {
  const int c = lane & 15, g = lane >> 4;
  f32x4 h1[4][2], h2[4][2], d1[4][2];
  mlp_bias(h1, h2, sv, lane);
  mlp_layer1(h1, TwinQL1{w1}, qh, lane);
#pragma unroll
  for (int hb = 0; hb < 4; ++hb) {
#pragma unroll
    for (int r = 0; r < 4; ++r) { h1[hb][0][r] = TwinQL1::act(h1[hb][0][r]); h1[hb][1][r] = TwinQL1::act(h1[hb][1][r]); }
  }
  mlp_layer2(h2, a2, h1);
  const float* sw = lds_here(sv);
  float P[2];
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    float q[4];
#pragma unroll
    for (int ho = 0; ho < 4; ++ho) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float w = sw[kMgW3 + 16 * ho + 4 * g + r], t = TwinQL1::act(h2[ho][b][r]);
        q[ho] = r == 0 ? w * t : fmaf(w, t, q[ho]);
        h2[ho][b][r] = TwinQL1::dact(t, w);  // dz2
      }
    }
    P[b] = (q[0] + q[1]) + (q[2] + q[3]);
    P[b] += __shfl_xor(P[b], 16);
    P[b] += __shfl_xor(P[b], 32);
    d1[0][b] = d1[1][b] = d1[2][b] = d1[3][b] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  }
  float a2t[4][4][4];
#pragma unroll
  for (int e = 0; e < 64; ++e) a2t[e >> 4][(e >> 2) & 3][e & 3] = w2t[64 * e + lane];
  mlp_layer2(d1, a2t, h2);  // W2^T dz2
  const float* wa = lds_here(wa0);
  float da[2][A];
#pragma unroll
  for (int b = 0; b < 2; ++b) {
#pragma unroll
    for (int j = 0; j < A; ++j) da[b][j] = 0.0f;
  }
#pragma unroll
  for (int hi = 0; hi < 4; ++hi) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int u = 16 * hi + 4 * g + r;
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const float d = TwinQL1::dact(h1[hi][b][r], d1[hi][b][r]);  // dz1
#pragma unroll
        for (int j = 0; j < A; ++j) da[b][j] = fmaf(wa[4 * u + j], d, da[b][j]);
      }
    }
  }
#pragma unroll
  for (int b = 0; b < 2; ++b) {
#pragma unroll
    for (int j = 0; j < A; ++j) {
      da[b][j] += __shfl_xor(da[b][j], 16);
      da[b][j] += __shfl_xor(da[b][j], 32);
      if (g == 0) dq[(16 * b + c) * kDpgQ + j] = da[b][j];
    }
    if (g == 0) dq[(16 * b + c) * kDpgQ + 4] = bias3 + P[b];
  }
}

// One wavefront per workgroup owns 64-row tiles of the minibatch and walks them grid-stride.  Per tile: gather the obs rows (index)
// through the LDS tile and forward them through pi (lane = row); a = clamp(pi) behind the observation in the critic's tile; Q1 and
// dQ1/da per half tile on the matrix cores; back on lane = row, dmu = -(1/B) dQ/da plus the smoothness deltas under the clamp mask,
// and up to three PpoNet::backward passes — on obs + noise (lam_S), on obs_next (lam_T) and on obs itself — into the same resident
// accumulators, exactly as ppo_actor_kernel orders them.  At the end the workgroup writes ONE partial vector.
//
// CT: the centralized (CTDE) form, Args = CtdeDpgArgs.  The critic's tile takes the other agent's observation rows at their columns
// (stage_rows, a second pointer array) and its action: supplied by minibatch position, or pi_{1-k} forward only on the lane's own row
// from LDS (PpoNet::forward of the pair's other size: (3,4,1) beside a (15,16,4) agent k and the reverse), clamped, before agent k's own pass so that it costs no
// register across the critic's phase.  Agent k's observation and action go to their own columns, `was` is fc1_w's columns of a_k.
// The other agent's action is a VALUE: no gradient for agent 1-k is produced (the reference's backward pass leaves one in that actor's
// .grad, which that agent zeroes before anything reads it; include/quadrotor_hip.h).
// Everything else is the one-agent walk; the whole body is ONE force-inlined function with the form as a compile-time argument,
// which leaves the one-agent kernels their registers, where hooks around the loss phase did not (§8.9).
template <int D, int H, int A, bool CT, class Args>
__device__ __forceinline__ void dpg_walk(const Args& a) {
  using Net = PpoNet<D, H, A>;
  using PY = PpoLayout<D, H, A>;
  using Y = DpgLayout<D, H, A>;
  constexpr int XS = Net::XS, HS = Net::HS;
  __shared__ float sm[Net::SM];
  __shared__ float xs[64 * XS], hs[64 * HS], ds[64 * kPpoDelta];
  __shared__ float qs[64 * kMgX], w1s[TwinQL1::SIZE], w2ts[64 * 64], svec[kTqVec], was[64 * 4], dq[64 * kDpgQ];
  __shared__ const float* src[64];
  __shared__ double red[64 * Y::NS];
  using Other = PpoNet<D == 15 ? 3 : 15, D == 15 ? 4 : 16, D == 15 ? 1 : 4>;  // (CT) the Decoupled pair's other half: its forward pass
  __shared__ const float* src1[CT ? 64 : 1];
  __shared__ float osm[CT ? Other::SM : 4];
  const int lane = threadIdx.x;
  const int QH = a.hidden;
  int IN = D + A, xcol = 0, acol = D;  // the critic's width, agent k's observation and action columns in its row
  if constexpr (CT) { IN = a.in_dim; xcol = a.col_own; acol = a.acol_own; }
  float a2[4][4][4];
  {
    float a2t[4][4][4];
    load_fc2(a2, a2t, a.q.fc2_w, QH, lane);
#pragma unroll
    for (int e = 0; e < 64; ++e) w2ts[64 * e + lane] = a2t[e >> 4][(e >> 2) & 3][e & 3];
  }
  twinq_fill_small(w1s, svec, a.q, IN, QH, lane);
#pragma unroll
  for (int j = 0; j < 4; ++j) was[4 * lane + j] = (lane < QH && j < A) ? a.q.fc1_w[lane * IN + acol + j] : 0.0f;
  if constexpr (CT) {
    if (!a.action_other) {
      PpoArgs p{};
      p.w = a.other;
      Other::fill(osm, p, lane);
    }
  }
  const float bias3 = a.q.fc3_b[0];
  Net net;
  net.zero();
  {
    PpoArgs p{};
    p.w = a.w;
    p.noise = a.noise;
    Net::fill(sm, p, lane);
  }
  for (int i = lane; i < 64 * XS; i += 64) xs[i] = (i % XS == D) ? 1.0f : 0.0f;  // the ones column; the rest of the padding stays zero
  for (int i = lane; i < 64 * HS; i += 64) hs[i] = (i % HS == H) ? 1.0f : 0.0f;
  for (int i = lane; i < 64 * kMgX; i += 64) qs[i] = 0.0f;                       // columns >= IN stay zero
  __syncthreads();
  float nominal[A];
#pragma unroll
  for (int j = 0; j < A; ++j) nominal[j] = a.nominal ? a.nominal[j] : 0.0f;
  double st[Y::NS];
#pragma unroll
  for (int q = 0; q < Y::NS; ++q) st[q] = 0.0;

  const int64_t tiles = (a.B + 63) / 64;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t row0 = tile * 64;
    const bool active = row0 + lane < a.B;
    int64_t i = active ? (a.index ? a.index[row0 + lane] : row0 + lane) : 0;
    i = i < 0 ? 0 : (i >= a.rows ? a.rows - 1 : i);  // never a read outside the buffer
    src[lane] = active ? a.obs + i * D : nullptr;
    if constexpr (CT) src1[lane] = active ? a.obs_other + i * a.od_other : nullptr;
    __syncthreads();
    ppo_stage<D, XS>(xs, src, lane);
    if constexpr (CT) stage_rows(qs, kMgX, src1, a.od_other, a.col_other, lane);
    __syncthreads();
    if constexpr (CT) {  // the other agent's action: a value only
      float* qa = qs + lane * kMgX + a.acol_other;
      if (a.action_other) {
        for (int f = 0; f < a.ad_other; ++f) qa[f] = active ? a.action_other[(row0 + lane) * a.ad_other + f] : 0.0f;
      } else {
        constexpr int OD = D == 15 ? 3 : 15, OA = D == 15 ? 1 : 4;
        constexpr int OH = D == 15 ? 4 : 16;
        float xo[OD], g1[OH], g2[OH], mo[OA];
#pragma unroll
        for (int k = 0; k < OD; ++k) xo[k] = qs[lane * kMgX + a.col_other + k];
        Other::forward(osm, xo, g1, g2, mo);
#pragma unroll
        for (int f = 0; f < OA; ++f) qa[f] = fminf(fmaxf(mo[f], -a.max_action), a.max_action);
      }
    }
    float x[D], h1[H], h2[H], mu[A], m[A], dm[A];
#pragma unroll
    for (int k = 0; k < D; ++k) x[k] = xs[lane * XS + k];
    Net::forward(sm, x, h1, h2, mu);
    // the critic's phase needs the registers: x waits in its tile (and in qs), pi's activations in the two tiles that are free
    // until the first backward pass
#pragma unroll
    for (int k = 0; k < D; ++k) qs[lane * kMgX + xcol + k] = x[k];
#pragma unroll
    for (int u = 0; u < H; ++u) { hs[lane * HS + u] = h1[u]; ds[lane * kPpoDelta + u] = h2[u]; }
#pragma unroll
    for (int j = 0; j < A; ++j) {
      m[j] = fminf(fmaxf(mu[j], -a.max_action), a.max_action);
      qs[lane * kMgX + acol + j] = m[j];
      if (active && fabsf(mu[j]) > a.max_action) st[1] += 1.0;
    }
    __syncthreads();
#pragma unroll 1
    for (int half = 0; half < 2; ++half)
      dpg_q1_half<A>(a2, lds_here(w2ts), qs + 32 * half * kMgX, lds_here(w1s), lds_here(svec), was, dq + 32 * half * kDpgQ, bias3, lane);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < H; ++u) { h1[u] = hs[lane * HS + u]; h2[u] = ds[lane * kPpoDelta + u]; }
    if (active) st[0] += (double)dq[lane * kDpgQ + 4];
#pragma unroll
    for (int j = 0; j < A; ++j) dm[j] = -a.inv_b * dq[lane * kDpgQ + j];  // d(-mean Q1) / da

    if (a.lam_M != 0.0f) {
#pragma unroll
      for (int j = 0; j < A; ++j) {
        const float d = m[j] - nominal[j];
        if (active) st[4] += (double)(d * d);
        dm[j] = fmaf(a.c_M, d, dm[j]);
      }
    }
    // a smoothness pass on other input rows y: the difference enters both ends — dm for x's pass, -c d for y's own, here
    auto other = [&](const float (&y)[D], float c, double& sum) {
      float g1[H], g2[H], mo[A], dmo[A];
      Net::forward(sm, y, g1, g2, mo);
#pragma unroll
      for (int j = 0; j < A; ++j) {
        const float d = m[j] - fminf(fmaxf(mo[j], -a.max_action), a.max_action);
        if (active) sum += (double)(d * d);
        dm[j] = fmaf(c, d, dm[j]);
        dmo[j] = (active && fabsf(mo[j]) <= a.max_action) ? -c * d : 0.0f;
      }
      net.backward(sm, xs, hs, ds, g1, g2, mo, dmo, lane);
    };
    if (a.lam_S != 0.0f) {
      float y[D];
#pragma unroll
      for (int k = 0; k < D; ++k) { y[k] = xs[lane * XS + k] + sm[Net::O_NOISE + k]; xs[lane * XS + k] = y[k]; }
      other(y, a.c_S, st[3]);
    }
    if (a.lam_T != 0.0f) {
      src[lane] = active ? a.obs_next + i * D : nullptr;
      __syncthreads();
      ppo_stage<D, XS>(xs, src, lane);
      __syncthreads();
      float y[D];
#pragma unroll
      for (int k = 0; k < D; ++k) y[k] = xs[lane * XS + k];
      other(y, a.c_T, st[2]);
    }
    if (a.lam_S != 0.0f || a.lam_T != 0.0f) {
#pragma unroll
      for (int k = 0; k < D; ++k) xs[lane * XS + k] = qs[lane * kMgX + xcol + k];
    }
    float dmu[A];
#pragma unroll
    for (int j = 0; j < A; ++j) dmu[j] = (active && fabsf(mu[j]) <= a.max_action) ? dm[j] : 0.0f;
    net.backward(sm, xs, hs, ds, h1, h2, mu, dmu, lane);  // (ends with a barrier: the tiles are free for the next rows)
  }

  double* P = a.partials + (int64_t)blockIdx.x * Y::NP;
  Net::template emit<D, Net::NB1>(P + PY::O_W1, P + PY::O_B1, net.acc1, H, lane);
  Net::template emit<H, Net::NBH>(P + PY::O_W2, P + PY::O_B2, net.acc2, H, lane);
  Net::template emit<H, Net::NBH>(P + PY::O_W3, P + PY::O_B3, net.acc3, A, lane);
  // the per-lane sums: across the lanes in lane order
#pragma unroll
  for (int q = 0; q < Y::NS; ++q) red[lane * Y::NS + q] = st[q];
  __syncthreads();
  if (lane < Y::NS) {
    double s = 0.0;
    for (int l = 0; l < 64; ++l) s += red[l * Y::NS + lane];
    P[Y::O_ST + lane] = s;
  }
}

template <int D, int H, int A>
__global__ __launch_bounds__(64) void dpg_actor_kernel(const DpgArgs a) { dpg_walk<D, H, A, false>(a); }

// Agent k of two under one centralized critic (qr_ctde_dpg_actor_grad): <15, 16, 4> for k = 0, <3, 4, 1> for k = 1.
template <int D, int H, int A>
__global__ __launch_bounds__(64) void ctde_dpg_actor_kernel(const CtdeDpgArgs a) { dpg_walk<D, H, A, true>(a); }

struct DpgReduceArgs {
  const double* partials;   // [n_parts][np]
  float* grad[6];           // fc1_w, fc1_b, fc2_w, fc2_b, mean_w, mean_b
  float* stats;             // [4]
  int32_t off[7];           // start of each gradient tensor in a partial vector; off[6] = the five sums
  int32_t n_parts, np;
  double B, BA;             // rows, rows x action_dim
  float lam_T, lam_S, lam_M;
};

// Workgroups 0 .. gridDim.x - 2: sixteen consecutive gradient entries each (reduce16_entries).  The last one: the five sums (256
// strided slices each, then a tree), and from them `stats`.
__global__ __launch_bounds__(256) void dpg_reduce_kernel(const DpgReduceArgs o) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  if (blockIdx.x + 1 < gridDim.x) {
    const int e = reduce16_entries(o.partials, o.n_parts, o.np, o.off[6], red);
    if (e >= 0) {
      const int k = entry_tensor<6>(e, o.off);
      float* dst = o.grad[0];
#pragma unroll
      for (int j = 1; j < 6; ++j)
        if (k == j) dst = o.grad[j];
      dst[e - o.off[k]] = (float)red[t];
    }
    return;
  }
  double s[5];
#pragma unroll
  for (int q = 0; q < 5; ++q) s[q] = block_sum_column(o.partials + o.off[6] + q, o.n_parts, o.np, red);
  if (t == 0) {
    const double reg = ((double)o.lam_T * s[2] + (double)o.lam_S * s[3] + (double)o.lam_M * s[4]) / o.BA;
    o.stats[0] = (float)(-s[0] / o.B + reg);
    o.stats[1] = (float)(s[0] / o.B);
    o.stats[2] = (float)(s[1] / o.BA);
    o.stats[3] = (float)reg;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// qr_soft_update
// ------------------------------------------------------------------------------------------------------------------
constexpr int kSoftMax = 24;   // a twin critic's twelve tensors and an actor's six, with room for a seven-tensor actor
constexpr int kSoftCols = 32;  // workgroups per tensor (of 256 threads, grid-stride over its entries)

struct SoftUpdateArgs {
  float* target[kSoftMax];
  const float* param[kSoftMax];
  int64_t count[kSoftMax];
  float tau, omt;              // float32(tau), float32(1.0 - tau) with the subtraction in double
};

// Workgroup row blockIdx.y owns one tensor.  target = tau * param + (1 - tau) * target as torch evaluates it: two products and a sum,
// each rounded on its own.  The library is built with -ffp-contract=fast, under which HIP's __fmul_rn / __fadd_rn are plain * and +
// and the code generator fuses them whatever the source says (the first build came out as v_mul_f32 + v_fmac_f32 and missed torch's
// bits): each product passes through an empty asm, which the sum cannot be fused across.
__device__ __forceinline__ float rounded(float v) {
  asm volatile("" : "+v"(v));
  return v;
}

__global__ __launch_bounds__(256) void soft_update_kernel(const SoftUpdateArgs a) {
  float* t = a.target[0];
  const float* p = a.param[0];
  int64_t n = a.count[0];
#pragma unroll
  for (int k = 1; k < kSoftMax; ++k)
    if ((int)blockIdx.y == k) { t = a.target[k]; p = a.param[k]; n = a.count[k]; }
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    t[i] = rounded(__fmul_rn(a.tau, p[i])) + rounded(__fmul_rn(a.omt, t[i]));
}

}  // namespace qr
