// qr_ppo.h — part of the gfx950 quadrotor step library (included by quadrotor_kernels.hip, after qr_critic.h).
// The actor half of one PPO minibatch update (PPO.train, algos/ppo/ppo.py:169-182, plus algos/policy_regularization.py): the
// clipped-surrogate loss with its three smoothness terms and the gradients with respect to MLP_Actor_PPO's seven tensors, read
// from the rollout storage in place: ppo_actor_kernel + ppo_reduce_kernel (qr_ppo_actor_grad).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "quadrotor_hip.h"
#include "qr_actor.h"

namespace qr {

struct PpoArgs {
  ActorW w;
  const float *obs, *final_obs;      // [T+1][N][D]; [T][N][D] or NULL
  const uint8_t *done, *truncated;   // [T][N][n_agents], [T][N] or NULL: read with final_obs only
  const float *action, *logp_old;    // row i at base + i * act_stride (the column offset is already applied)
  const float* advantage;            // element i at advantage[i * adv_stride]
  const int64_t* index;              // [B] or NULL (rows 0..B-1)
  const float *noise, *nominal;      // [D], [A]
  double* partials;                  // [grid][NP]
  int64_t B, N, rows;                // rows = T * N
  int32_t act_stride, adv_stride, n_agents;
  float clip, max_action;
  float lam_T, lam_S, lam_M;         // only their being zero is read here (wave-uniform branches)
  float inv_b, c_T, c_S, c_M;        // 1 / B and 2 lam / (B A): the per-row factors of the gradient
};

// Layout of one workgroup's partial vector = the order of the seven gradient tensors, then the six sums of `stats`.
template <int D, int H, int A>
struct PpoLayout {
  static constexpr int O_W1 = 0, O_B1 = O_W1 + H * D, O_W2 = O_B1 + H, O_B2 = O_W2 + H * H, O_W3 = O_B2 + H, O_B3 = O_W3 + A * H,
                       O_LS = O_B3 + A, O_ST = O_LS + A, NP = O_ST + 6;
};
// sums: 0 S_i, 1 rows with rho outside the clip range, 2 (rho - 1) - log rho, 3 / 4 / 5 the squared differences of the temporal,
// spatial and magnitude terms
constexpr int kPpoDelta = 17;  // row stride of the delta tile (16 columns; odd: a lane's own row is conflict-free)

// One lane = one row for the forward pass and the deltas (input-major VALU layers, weights broadcast from LDS, as ActorLds);
// the WEIGHT GRADIENTS are the contractions over rows  dW[out][in] = sum_rows delta[row][out] act[row][in]  and run on
// v_mfma_f32_16x16x4_f32 with k over the tile's 64 rows (16 k-steps), from two LDS tiles the lanes write their rows into:
//   lane l: c = l & 15, g = l >> 4.   A[c][k = g] = delta[row 4 s + g][c],  B[k = g][c] = act[row 4 s + g][16 blk + c],
//   D: lane holds dW[4 g + r][16 blk + c], r = 0..3.
// The activation tile carries a column of ones behind its K real columns, so that column K of the product is the bias gradient;
// columns past that are zero.  A layer narrower than 16 (the 3 -> 4 -> 4 -> 1 agent) is the same code on zero-padded tiles.
// The accumulators stay in registers over all of a wave's tiles.
template <int D, int H, int A>
struct PpoNet {
  using Y = PpoLayout<D, H, A>;
  static constexpr int NB1 = (D + 16) / 16, NBH = (H + 16) / 16;  // 16-column blocks of an activation tile, ones column included
  static constexpr int XS = 16 * NB1 + 1, HS = 16 * NBH + 1;      // row strides (odd)
  // The weights in LDS.  Forward: TRANSPOSED to [in][out] (out padded to a multiple of 4), so that a layer runs input-major with
  // broadcast ds_read_b128 (ActorLds's layout; its own code is not instantiated here, so that no kernel of the rollout shares a
  // function with this one).  Backward: fc2_w and mean_w as they are, [out][in] — W^T delta is input-major over `out`.
  static constexpr int HP = (H + 3) & ~3, AP = (A + 3) & ~3;
  static constexpr int O_FC1W = 0, O_FC1B = O_FC1W + D * HP, O_FC2W = O_FC1B + HP, O_FC2B = O_FC2W + H * HP, O_MW = O_FC2B + HP,
                       O_MB = O_MW + H * AP, O_LS = O_MB + AP, O_BW2 = O_LS + AP, O_BW3 = O_BW2 + H * H, O_NOISE = O_BW3 + A * H,
                       SM = O_NOISE + D;
  static_assert(H <= 16 && A <= 4 && H % 4 == 0, "one 16-row MFMA block per layer");

  f32x4 acc1[NB1], acc2[NBH], acc3[NBH];

  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int b = 0; b < NB1; ++b) acc1[b] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int b = 0; b < NBH; ++b) { acc2[b] = f32x4{0.0f, 0.0f, 0.0f, 0.0f}; acc3[b] = f32x4{0.0f, 0.0f, 0.0f, 0.0f}; }
  }

  __device__ static void fill(float* sm, const PpoArgs& a, int lane) {
    const ActorW& p = a.w;
    for (int i = lane; i < D * HP; i += 64) { const int k = i / HP, j = i - k * HP; sm[O_FC1W + i] = j < H ? p.fc1_w[j * D + k] : 0.0f; }
    for (int i = lane; i < H * HP; i += 64) { const int k = i / HP, j = i - k * HP; sm[O_FC2W + i] = j < H ? p.fc2_w[j * H + k] : 0.0f; }
    for (int i = lane; i < H * AP; i += 64) { const int k = i / AP, j = i - k * AP; sm[O_MW + i] = j < A ? p.mean_w[j * H + k] : 0.0f; }
    if (lane < HP) { sm[O_FC1B + lane] = lane < H ? p.fc1_b[lane] : 0.0f; sm[O_FC2B + lane] = lane < H ? p.fc2_b[lane] : 0.0f; }
    if (lane < AP) { sm[O_MB + lane] = lane < A ? p.mean_b[lane] : 0.0f; sm[O_LS + lane] = lane < A ? p.log_std[lane] : 0.0f; }
    for (int i = lane; i < H * H; i += 64) sm[O_BW2 + i] = p.fc2_w[i];
    for (int i = lane; i < A * H; i += 64) sm[O_BW3 + i] = p.mean_w[i];
    for (int i = lane; i < D; i += 64) sm[O_NOISE + i] = a.noise ? a.noise[i] : 0.0f;
  }

  template <int NI, int NO, int NOP>
  __device__ __forceinline__ static void layer(const float* w, const float* bias, const float (&x)[NI], float (&y)[NO]) {
#pragma unroll
    for (int j = 0; j < NO; ++j) y[j] = bias[j];
#pragma unroll
    for (int k = 0; k < NI; ++k) {
#pragma unroll
      for (int j = 0; j < NO; ++j) y[j] = fmaf(w[k * NOP + j], x[k], y[j]);
    }
  }

  // (The weights are read from LDS where they are used, in every pass: an offset the compiler cannot see through keeps it from
  //  hoisting the loop-invariant reads out of the tile loop into ~800 registers.)
  __device__ __forceinline__ static const float* here(const float* sm) {
    int z = 0;
    asm volatile("" : "+v"(z));
    return sm + z;
  }

  __device__ __forceinline__ static void forward(const float* sm0, const float (&x)[D], float (&h1)[H], float (&h2)[H], float (&mu)[A]) {
    const float* sm = here(sm0);
    layer<D, H, HP>(sm + O_FC1W, sm + O_FC1B, x, h1);
#pragma unroll
    for (int j = 0; j < H; ++j) h1[j] = fmaxf(h1[j], 0.0f);
    layer<H, H, HP>(sm + O_FC2W, sm + O_FC2B, h1, h2);
#pragma unroll
    for (int j = 0; j < H; ++j) h2[j] = fmaxf(h2[j], 0.0f);
    float pre[A];
    layer<H, A, AP>(sm + O_MW, sm + O_MB, h2, pre);
#pragma unroll
    for (int j = 0; j < A; ++j) mu[j] = tanh_fast(pre[j]);
  }

  template <int NB, int STRIDE>
  __device__ __forceinline__ static void wgrad(const float* ds, const float* act, f32x4 (&acc)[NB], int lane) {
    const int c = lane & 15, g = lane >> 4;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const float a = ds[(4 * s + g) * kPpoDelta + c];
#pragma unroll
      for (int b = 0; b < NB; ++b) acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, act[(4 * s + g) * STRIDE + 16 * b + c], acc[b], 0, 0, 0);
    }
  }

  template <int NV>
  __device__ __forceinline__ static void put_delta(float* ds, const float (&d)[NV], int lane) {
#pragma unroll
    for (int j = 0; j < 16; ++j) ds[lane * kPpoDelta + j] = j < NV ? d[j] : 0.0f;
  }

  // One pass backwards from dmu = dLoss / dmu of the lane's row (0 on a row that does not count).  xs holds the pass's input rows.
  __device__ __forceinline__ void backward(const float* sm0, const float* xs, float* hs, float* ds, const float (&h1)[H], const float (&h2)[H],
                                           const float (&mu)[A], const float (&dmu)[A], int lane) {
    float dp[A], dz2[H], dz1[H];
    const float* sm = here(sm0);
#pragma unroll
    for (int j = 0; j < A; ++j) dp[j] = dmu[j] * fmaf(-mu[j], mu[j], 1.0f);
    put_delta<A>(ds, dp, lane);
#pragma unroll
    for (int u = 0; u < H; ++u) hs[lane * HS + u] = h2[u];
    __syncthreads();
    wgrad<NBH, HS>(ds, hs, acc3, lane);
#pragma unroll
    for (int u = 0; u < H; ++u) dz2[u] = 0.0f;
#pragma unroll
    for (int j = 0; j < A; ++j) {
#pragma unroll
      for (int u = 0; u < H; ++u) dz2[u] = fmaf(sm[O_BW3 + j * H + u], dp[j], dz2[u]);
    }
#pragma unroll
    for (int u = 0; u < H; ++u) dz2[u] = h2[u] > 0.0f ? dz2[u] : 0.0f;
    __syncthreads();  // both tiles are read
    put_delta<H>(ds, dz2, lane);
#pragma unroll
    for (int u = 0; u < H; ++u) hs[lane * HS + u] = h1[u];
    __syncthreads();
    wgrad<NBH, HS>(ds, hs, acc2, lane);
#pragma unroll
    for (int u = 0; u < H; ++u) dz1[u] = 0.0f;
#pragma unroll
    for (int j = 0; j < H; ++j) {
#pragma unroll
      for (int u = 0; u < H; ++u) dz1[u] = fmaf(sm[O_BW2 + j * H + u], dz2[j], dz1[u]);
    }
#pragma unroll
    for (int u = 0; u < H; ++u) dz1[u] = h1[u] > 0.0f ? dz1[u] : 0.0f;
    __syncthreads();
    put_delta<H>(ds, dz1, lane);
    __syncthreads();
    wgrad<NB1, XS>(ds, xs, acc1, lane);
    __syncthreads();
  }

  // dW[out][in] (in < K) and db[out] (in == K) of one layer into the workgroup's partial vector
  template <int K, int NB>
  __device__ __forceinline__ static void emit(double* w, double* b, const f32x4 (&acc)[NB], int n_out, int lane) {
    const int c = lane & 15, g = lane >> 4;
#pragma unroll
    for (int blk = 0; blk < NB; ++blk) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int out = 4 * g + r, in = 16 * blk + c;
        if (out < n_out && in < K) w[out * K + in] = (double)acc[blk][r];
        if (out < n_out && in == K) b[out] = (double)acc[blk][r];
      }
    }
  }
};

// The rows src[r][0..D) of a tile into xs (row stride XS): linear dword loads along each row, eight in flight per lane; a NULL
// row (past the batch) is zeros.
template <int D, int XS>
__device__ __forceinline__ void ppo_stage(float* xs, const float* const* src, int lane) {
#pragma unroll
  for (int u0 = 0; u0 < D; u0 += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (u0 + u < D) {
        const int e = 64 * (u0 + u) + lane, r = e / D, k = e - r * D;
        const float* p = src[r];
        v[u] = p ? p[k] : 0.0f;
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (u0 + u < D) {
        const int e = 64 * (u0 + u) + lane, r = e / D, k = e - r * D;
        xs[r * XS + k] = v[u];
      }
    }
  }
}

// One wavefront per workgroup owns 64-row tiles of the minibatch and walks them grid-stride.  Per tile: gather the rows (index)
// through the LDS tile, forward, the per-row loss terms, then up to three backward passes — on x + noise (lam_S), on obs_next
// (lam_T; critic_kernel<NEXT>'s rule: final_obs where the env was re-sampled, obs[i + N] elsewhere) and on x itself — each adding
// into the same resident accumulators.  At the end the workgroup writes ONE partial vector; ppo_reduce_kernel sums them.
template <int D, int H, int A>
__global__ __launch_bounds__(64) void ppo_actor_kernel(const PpoArgs a) {
  using Net = PpoNet<D, H, A>;
  using Y = PpoLayout<D, H, A>;
  constexpr int XS = Net::XS, HS = Net::HS;
  __shared__ float sm[Net::SM];
  __shared__ float xs[64 * XS], hs[64 * HS], ds[64 * kPpoDelta];
  __shared__ const float* src[64];
  __shared__ double red[64 * (A + 6)];
  const int lane = threadIdx.x;
  Net net;
  net.zero();
  Net::fill(sm, a, lane);
  for (int i = lane; i < 64 * XS; i += 64) xs[i] = (i % XS == D) ? 1.0f : 0.0f;  // the ones column; the rest of the padding stays zero
  for (int i = lane; i < 64 * HS; i += 64) hs[i] = (i % HS == H) ? 1.0f : 0.0f;
  __syncthreads();
  float ls[A], ivar[A], nominal[A];
#pragma unroll
  for (int j = 0; j < A; ++j) {
    ls[j] = sm[Net::O_LS + j];
    ivar[j] = expf(-2.0f * ls[j]);
    nominal[j] = a.nominal ? a.nominal[j] : 0.0f;
  }
  const float lo = 1.0f - a.clip, hi = 1.0f + a.clip;
  double gls[A], st[6];
#pragma unroll
  for (int j = 0; j < A; ++j) gls[j] = 0.0;
#pragma unroll
  for (int q = 0; q < 6; ++q) st[q] = 0.0;

  const int64_t tiles = (a.B + 63) / 64;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t row0 = tile * 64;
    const bool active = row0 + lane < a.B;
    int64_t i = active ? (a.index ? a.index[row0 + lane] : row0 + lane) : 0;
    i = i < 0 ? 0 : (i >= a.rows ? a.rows - 1 : i);  // never a read outside the storage
    src[lane] = active ? a.obs + i * D : nullptr;
    __syncthreads();
    ppo_stage<D, XS>(xs, src, lane);
    __syncthreads();
    float x[D], h1[H], h2[H], mu[A];
#pragma unroll
    for (int k = 0; k < D; ++k) x[k] = xs[lane * XS + k];
    Net::forward(sm, x, h1, h2, mu);

    // ppo.py:169-177 for the lane's row
    const float adv = a.advantage[i * a.adv_stride];
    float lp = 0.0f, old = 0.0f, diff[A];
#pragma unroll
    for (int j = 0; j < A; ++j) {
      diff[j] = a.action[i * a.act_stride + j] - mu[j];
      lp += fmaf(-0.5f * diff[j] * diff[j], ivar[j], -ls[j] - 0.91893853320467274f);
      old += a.logp_old[i * a.act_stride + j];
    }
    const float rho = expf(lp - old), s1 = rho * adv, s2 = fminf(fmaxf(rho, lo), hi) * adv;
    const bool inside = rho >= lo && rho <= hi;
    // torch.min splits a tie, and inside the range both halves arrive; outside it only the unclipped branch carries a gradient
    const float gS = (active && (inside || s1 < s2)) ? -a.inv_b * s1 : 0.0f;
    float m[A], dm[A], dmu[A];
#pragma unroll
    for (int j = 0; j < A; ++j) {
      dmu[j] = gS * diff[j] * ivar[j];
      if (active) gls[j] += (double)(gS * fmaf(diff[j] * diff[j], ivar[j], -1.0f));
      m[j] = fminf(fmaxf(mu[j], -a.max_action), a.max_action);
      dm[j] = 0.0f;
    }
    if (active) {
      st[0] += (double)fminf(s1, s2);
      st[1] += inside ? 0.0 : 1.0;
      st[2] += (double)((rho - 1.0f) - (lp - old));
    }
    if (a.lam_M != 0.0f) {
#pragma unroll
      for (int j = 0; j < A; ++j) {
        const float d = m[j] - nominal[j];
        if (active) st[5] += (double)(d * d);
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
      for (int k = 0; k < D; ++k) { y[k] = x[k] + sm[Net::O_NOISE + k]; xs[lane * XS + k] = y[k]; }
      other(y, a.c_S, st[4]);
    }
    if (a.lam_T != 0.0f) {
      bool reset = false;
      if (a.final_obs) {
        for (int k = 0; k < a.n_agents; ++k) reset |= a.done[i * a.n_agents + k] != 0;
        if (a.truncated) reset |= a.truncated[i] != 0;
      }
      src[lane] = !active ? nullptr : (reset ? a.final_obs + i * D : a.obs + (i + a.N) * D);
      __syncthreads();
      ppo_stage<D, XS>(xs, src, lane);
      __syncthreads();
      float y[D];
#pragma unroll
      for (int k = 0; k < D; ++k) y[k] = xs[lane * XS + k];
      other(y, a.c_T, st[3]);
    }
    if (a.lam_S != 0.0f || a.lam_T != 0.0f) {
#pragma unroll
      for (int k = 0; k < D; ++k) xs[lane * XS + k] = x[k];
    }
#pragma unroll
    for (int j = 0; j < A; ++j) dmu[j] += (active && fabsf(mu[j]) <= a.max_action) ? dm[j] : 0.0f;
    net.backward(sm, xs, hs, ds, h1, h2, mu, dmu, lane);  // (ends with a barrier: the tiles are free for the next rows)
  }

  double* P = a.partials + (int64_t)blockIdx.x * Y::NP;
  Net::template emit<D, Net::NB1>(P + Y::O_W1, P + Y::O_B1, net.acc1, H, lane);
  Net::template emit<H, Net::NBH>(P + Y::O_W2, P + Y::O_B2, net.acc2, H, lane);
  Net::template emit<H, Net::NBH>(P + Y::O_W3, P + Y::O_B3, net.acc3, A, lane);
  // the per-lane sums: across the lanes in lane order
#pragma unroll
  for (int j = 0; j < A; ++j) red[lane * (A + 6) + j] = gls[j];
#pragma unroll
  for (int q = 0; q < 6; ++q) red[lane * (A + 6) + A + q] = st[q];
  __syncthreads();
  if (lane < A + 6) {
    double s = 0.0;
    for (int l = 0; l < 64; ++l) s += red[l * (A + 6) + lane];
    P[Y::O_LS + lane] = s;
  }
}

struct PpoReduceArgs {
  const double* partials;   // [n_parts][np]
  float* grad[7];           // fc1_w, fc1_b, fc2_w, fc2_b, mean_w, mean_b, log_std
  float* stats;             // [4]
  const float* log_std;
  int32_t off[8];           // start of each gradient tensor in a partial vector; off[7] = the six sums
  int32_t n_parts, np, action_dim;
  double B;
  float entropy_coef, lam_T, lam_S, lam_M;
  const float* entropy_coef_dev;   // null: `entropy_coef` above; else the coefficient is *entropy_coef_dev (read only: qr_ppo_actor_grad_dev)
};

// Entry e of the result = the sum over the partial vectors of entry e, in float64 and in an order the grid alone fixes: Q entries
// per workgroup, 256 / Q slices of the partials each, then a tree over the slices.  Returns the sum in the threads of slice 0.
template <int Q>
__device__ __forceinline__ double ppo_block_sum(const PpoReduceArgs& o, double* red, int e, bool valid) {
  const int t = threadIdx.x, s = t / Q;
  double sum = 0.0;
  if (valid)
    for (int p = s; p < o.n_parts; p += 256 / Q) sum += o.partials[(int64_t)p * o.np + e];
  red[t] = sum;
  __syncthreads();
  for (int w = 128 / Q; w >= 1; w >>= 1) {
    if (s < w) red[t] += red[t + Q * w];
    __syncthreads();
  }
  return red[t];
}

// Workgroups 0 .. gridDim.x - 2: four gradient entries each.  The last one: the six sums, and from them `stats`.
__global__ __launch_bounds__(256) void ppo_reduce_kernel(const PpoReduceArgs o) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  if (blockIdx.x + 1 < gridDim.x) {
    const int e = 4 * blockIdx.x + (t & 3);
    const bool valid = e < o.off[7];
    const double v = ppo_block_sum<4>(o, red, e, valid);
    if (t < 4 && valid) {
      float* dst = o.grad[0];
      int base = 0;
#pragma unroll
      for (int k = 1; k < 7; ++k)
        if (e >= o.off[k]) { dst = o.grad[k]; base = o.off[k]; }
      const float entropy_coef = o.entropy_coef_dev ? *o.entropy_coef_dev : o.entropy_coef;
      dst[e - base] = (float)(e >= o.off[6] ? v - (double)entropy_coef : v);  // dH / dlog_std = 1 per component
    }
    return;
  }
  const bool valid = (t & 7) < 6;
  ppo_block_sum<8>(o, red, o.off[7] + (t & 7), valid);
  if (t == 0) {
    const double na = o.B * o.action_dim;
    const float entropy_coef = o.entropy_coef_dev ? *o.entropy_coef_dev : o.entropy_coef;
    double H = 0.0;
    for (int j = 0; j < o.action_dim; ++j) H += 0.5 + 0.91893853320467274 + (double)o.log_std[j];
    const double reg = ((double)o.lam_T * red[3] + (double)o.lam_S * red[4] + (double)o.lam_M * red[5]) / na;
    o.stats[0] = (float)(-red[0] / o.B - (double)entropy_coef * H + reg);
    o.stats[1] = (float)(red[0] / o.B);
    o.stats[2] = (float)(red[1] / o.B);
    o.stats[3] = (float)(red[2] / o.B);
  }
}

}  // namespace qr
