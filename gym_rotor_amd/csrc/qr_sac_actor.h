// qr_sac_actor.h — part of the gfx950 quadrotor step library (included by quadrotor_kernels.hip only, after qr_sac.h).
// The actor half of one SAC minibatch update (SAC.train, algos/sac/sac.py:182-211, the non-CTDE branch without the spectral-norm
// term, plus algos/policy_regularization.py with rl_algo == "SAC" and MLP_Actor_SAC.sample, algos/sac/sac_mlp.py:55-79):
//   sac_actor_kernel + sac_actor_reduce_kernel (qr_sac_actor_grad)
//       loss = mean_j (alpha logp_j - min(Q1, Q2)(obs[i], a_j)) + lam_T mse(r, rn) + lam_S mse(r, rp) + lam_M mse(r, nominal)
//   with FOUR independent samples of pi (the loss pass; the regulariser's own sample r; on obs_next; on obs + noise), its gradients for
//   MLP_Actor_SAC's eight tensors, and what alpha's own update needs, -(target_entropy + mean_j logp_j).
//   ctde_sac_actor_kernel + sac_actor_reduce_kernel (qr_ctde_sac_actor_grad)   the same for agent k of two under ONE centralized (CTDE)
//   twin critic (sac.py:175-203): the other agent's action as a value, logp from a second sample of agent k; the same walk blocks.
// The pieces are shared: the actor's layers, MFMA weight gradients, delta tile and emit are PpoNet's static pieces (qr_ppo.h), a critic's
// forward pass and dQ/da are dpg_q1_half (qr_td3_actor.h), the reduction is reduce16_entries / block_sum_column.  New here:
//   - the two-headed passes (SacNet): forward keeps the pre-tanh mean and log_std_linear's output; backward puts dmean in columns
//     [0, A) and dlog_std in [4, 4 + A) of the delta tile, so ONE wgrad over h2 yields both heads' weight gradients, and dz2
//     contracts both heads' weights;
//   - the second critic: Q1 and Q2 run one after the other through ONE set of LDS arrays and ONE resident fc2_w, refilled from L2 per
//     tile (a second set does not fit under 64 KB of LDS beside the actor's tiles);
//   - the selection min(Q1, Q2) per row, with torch's half-and-half on an exact tie.
// The tile walk is separate from ppo_actor_kernel's and dpg_walk's (qr_td3_actor.h says why those two are apart), but the two kernels
// here are built from ONE set of force-inlined blocks — sac_prologue, sac_row_index / sac_noise_row, sac_critics, sac_select,
// sac_regularize, sac_epilogue — so a fix to a block reaches both.  Each kernel keeps its own __shared__ arrays and the glue between the blocks.
// 1 - a^2 and a come from t = exp(-2|u|) as in qr_sac.h (never from the rounded a), -eps^2/2 from eps.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "quadrotor_hip.h"
#include "qr_ppo.h"
#include "qr_td3.h"
#include "qr_td3_actor.h"

namespace qr {

struct SacActorArgs {
  ActorW w;                          // pi: both heads (ls_w, ls_b); log_std points at readable floats (PpoNet::fill copies them)
  MlpNetW q[2];                      // Q1, Q2
  const float *obs, *obs_next;       // [>= rows][D]; obs_next is read with lam_T != 0 only
  const int64_t* index;              // [B] or NULL (rows 0..B-1)
  const float* eps[4];               // loss, reg, next, pert: [B][A] by minibatch position, or NULL: zeros
  const float *noise, *nominal;      // [D], [A]
  const float* alpha_dev;            // device scalar, or NULL: `alpha`
  double* partials;                  // [grid][NP]
  int64_t B, rows;
  int32_t hidden;                    // of the critics
  float alpha, max_action;
  float lam_T, lam_S, lam_M;         // only their being zero is read here (wave-uniform branches)
  float inv_b, c_T, c_S, c_M;        // 1 / B and 2 lam / (B A): the per-row factors of the gradient
};

// The centralized (CTDE) form for agent k of two (qr_ctde_sac_actor_grad): SacActorArgs' members are agent k's (w = pi_k, obs / obs_next /
// noise / nominal its own, eps[0] its first draw), q = the centralized twin critic whose row is [obs_0 | obs_1 | a_0 | a_1].
struct CtdeSacActorArgs : SacActorArgs {
  ActorW other;                      // pi_{1-k}, both heads, forward only; read when action_other is NULL
  const float* obs_other;            // [>= rows][od_other]
  const float* action_other;         // [B][ad_other] by minibatch position, used as it is, or NULL: tanh of pi_{1-k}'s sample
  const float* eps_other;            // [B][ad_other] by minibatch position: the other agent's draw, or NULL: zeros
  const float* eps_logp;             // [B][A] by minibatch position: agent k's SECOND draw (logp), or NULL: one sample, drawn with eps[0]
  int32_t od_other, ad_other;        // the other agent's widths
  int32_t col_own, col_other;        // first column of each agent's observation in the critic's row
  int32_t acol_own, acol_other;      // first column of each agent's action: D + off_k, D + off_{1-k}
  int32_t in_dim;                    // the row's width, <= 28
};

// One workgroup's partial vector: PpoLayout's six weight and bias tensors, log_std_linear's two, then the seven sums of `stats`:
// 0 min(Q1, Q2), 1 logp of the loss pass, 2 / 3 / 4 the squared differences of the temporal, spatial and magnitude terms,
// 5 log_std components of the loss pass outside [-20, 2], 6 rows that took Q2
template <int D, int H, int A>
struct SacLayout {
  static constexpr int O_LW = PpoLayout<D, H, A>::O_LS, O_LB = O_LW + A * H, O_ST = O_LB + A, NS = 7, NP = O_ST + NS;
};

// MLP_Actor_SAC beside PpoNet<D, H, A>: PpoNet's LDS block (fc1, fc2, the mean head, the backward copies, the noise row) is filled
// and read as it is; log_std_linear lives in a block of its own (sl): forward [H][AP] transposed, its bias, backward [A][H] as it is.
template <int D, int H, int A>
struct SacNet {
  using Net = PpoNet<D, H, A>;
  static constexpr int HS = Net::HS, XS = Net::XS, HP = Net::HP, AP = Net::AP;
  static constexpr int O_LW = 0, O_LB = O_LW + H * AP, O_BL = O_LB + AP, SL = O_BL + A * H;

  f32x4 acc1[Net::NB1], acc2[Net::NBH], acc3[Net::NBH];  // acc3: rows [0, A) mean_linear, rows [4, 4 + A) log_std_linear

  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int b = 0; b < Net::NB1; ++b) acc1[b] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int b = 0; b < Net::NBH; ++b) { acc2[b] = f32x4{0.0f, 0.0f, 0.0f, 0.0f}; acc3[b] = f32x4{0.0f, 0.0f, 0.0f, 0.0f}; }
  }

  __device__ static void fill(float* sl, const ActorW& p, int lane) {
    for (int i = lane; i < H * AP; i += 64) { const int k = i / AP, j = i - k * AP; sl[O_LW + i] = j < A ? p.ls_w[j * H + k] : 0.0f; }
    if (lane < AP) sl[O_LB + lane] = lane < A ? p.ls_b[lane] : 0.0f;
    for (int i = lane; i < A * H; i += 64) sl[O_BL + i] = p.ls_w[i];
  }

  // PpoNet::forward's sibling: the pre-tanh mean and log_std_linear's raw output
  __device__ __forceinline__ static void forward(const float* sm0, const float* sl0, const float (&x)[D], float (&h1)[H], float (&h2)[H],
                                                 float (&mean)[A], float (&lsr)[A]) {
    const float* sm = Net::here(sm0);
    const float* sl = Net::here(sl0);
    Net::template layer<D, H, HP>(sm + Net::O_FC1W, sm + Net::O_FC1B, x, h1);
#pragma unroll
    for (int j = 0; j < H; ++j) h1[j] = fmaxf(h1[j], 0.0f);
    Net::template layer<H, H, HP>(sm + Net::O_FC2W, sm + Net::O_FC2B, h1, h2);
#pragma unroll
    for (int j = 0; j < H; ++j) h2[j] = fmaxf(h2[j], 0.0f);
    Net::template layer<H, A, AP>(sm + Net::O_MW, sm + Net::O_MB, h2, mean);
    Net::template layer<H, A, AP>(sl + O_LW, sl + O_LB, h2, lsr);
  }

  // One pass backwards from dmean and dls = dLoss / d(mean, raw log_std) of the lane's row (0 on a row that does not count).
  // xs holds the pass's input rows.  PpoNet::backward's sibling: both heads share the first delta tile.
  __device__ __forceinline__ void backward(const float* sm0, const float* sl0, const float* xs, float* hs, float* ds, const float (&h1)[H],
                                           const float (&h2)[H], const float (&dmean)[A], const float (&dls)[A], int lane) {
    float d8[8], dz2[H], dz1[H];
    const float* sm = Net::here(sm0);
    const float* sl = Net::here(sl0);
#pragma unroll
    for (int j = 0; j < 4; ++j) { d8[j] = j < A ? dmean[j < A ? j : 0] : 0.0f; d8[4 + j] = j < A ? dls[j < A ? j : 0] : 0.0f; }
    Net::template put_delta<8>(ds, d8, lane);
#pragma unroll
    for (int u = 0; u < H; ++u) hs[lane * HS + u] = h2[u];
    __syncthreads();
    Net::template wgrad<Net::NBH, HS>(ds, hs, acc3, lane);
#pragma unroll
    for (int u = 0; u < H; ++u) dz2[u] = 0.0f;
#pragma unroll
    for (int j = 0; j < A; ++j) {
#pragma unroll
      for (int u = 0; u < H; ++u) dz2[u] = fmaf(sl[O_BL + j * H + u], dls[j], fmaf(sm[Net::O_BW3 + j * H + u], dmean[j], dz2[u]));
    }
#pragma unroll
    for (int u = 0; u < H; ++u) dz2[u] = h2[u] > 0.0f ? dz2[u] : 0.0f;
    __syncthreads();  // both tiles are read
    Net::template put_delta<H>(ds, dz2, lane);
#pragma unroll
    for (int u = 0; u < H; ++u) hs[lane * HS + u] = h1[u];
    __syncthreads();
    Net::template wgrad<Net::NBH, HS>(ds, hs, acc2, lane);
#pragma unroll
    for (int u = 0; u < H; ++u) dz1[u] = 0.0f;
#pragma unroll
    for (int j = 0; j < H; ++j) {
#pragma unroll
      for (int u = 0; u < H; ++u) dz1[u] = fmaf(sm[Net::O_BW2 + j * H + u], dz2[j], dz1[u]);
    }
#pragma unroll
    for (int u = 0; u < H; ++u) dz1[u] = h1[u] > 0.0f ? dz1[u] : 0.0f;
    __syncthreads();
    Net::template put_delta<H>(ds, dz1, lane);
    __syncthreads();
    Net::template wgrad<Net::NB1, XS>(ds, xs, acc1, lane);
    __syncthreads();
  }

  // log_std_linear's rows of acc3 (PpoNet::emit writes rows [0, n_out), mean_linear's): rows [4, 4 + A)
  __device__ __forceinline__ static void emit_head2(double* w, double* b, const f32x4 (&acc)[Net::NBH], int lane) {
    const int c = lane & 15, g = lane >> 4;
#pragma unroll
    for (int blk = 0; blk < Net::NBH; ++blk) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int out = 4 * g + r - 4, in = 16 * blk + c;
        if (out >= 0 && out < A && in < H) w[out * H + in] = (double)acc[blk][r];
        if (out >= 0 && out < A && in == H) b[out] = (double)acc[blk][r];
      }
    }
  }
};

// One row's sample (sac_mlp.py:65-76) from the heads' outputs and its noise, with what the backward pass needs
template <int A>
struct SacRow {
  float act[A];    // a = tanh(u)
  float om[A];     // 1 - a^2 = 4 t / (1 + t)^2
  float se[A];     // exp(ls) eps = du / dls
  bool in[A];      // -20 <= raw log_std <= 2: the clamp passes the gradient (at the bounds too, as torch's)
  float logp;

  __device__ __forceinline__ void sample(const float (&mean)[A], const float (&lsr)[A], const float (&e)[A]) {
    logp = 0.0f;
#pragma unroll
    for (int j = 0; j < A; ++j) {
      in[j] = lsr[j] >= -20.0f && lsr[j] <= 2.0f;
      const float ls = fminf(fmaxf(lsr[j], -20.0f), 2.0f);
      se[j] = expf(ls) * e[j];
      const float u = mean[j] + se[j];
      const float t = expf(-2.0f * fabsf(u));
      const float r = 1.0f / (1.0f + t);
      act[j] = copysignf((1.0f - t) * r, u);
      om[j] = 4.0f * t * r * r;
      logp += fmaf(-0.5f * e[j], e[j], -ls - 0.91893853320467274f) - logf(om[j] + 1e-6f);
    }
  }

  // dmean, dls from ga = dLoss / da and gl = dLoss / dlogp:  da/du = 1 - a^2,  dlogp/du = 2 a (1 - a^2) / (1 - a^2 + 1e-6),
  // du/dmean = 1, du/dls = exp(ls) eps and dlogp/dls = -1, both under the clamp's gate
  __device__ __forceinline__ void deltas(const float (&ga)[A], float gl, bool active, float (&dmean)[A], float (&dls)[A]) const {
#pragma unroll
    for (int j = 0; j < A; ++j) {
      const float du = fmaf(ga[j], om[j], gl * (2.0f * act[j] * om[j] / (om[j] + 1e-6f)));
      dmean[j] = active ? du : 0.0f;
      dls[j] = (active && in[j]) ? fmaf(du, se[j], -gl) : 0.0f;
    }
  }
};

// ---- The blocks of the tile walk that sac_actor_kernel and ctde_sac_actor_kernel are both built from.  Each is force-inlined into
// the kernel that owns the __shared__ arrays and takes them as plain pointers.  The one-agent kernel passes the critics' row as the
// constants IN = D + A, xcol = 0, acol = D; the CTDE kernel reads them from its arguments.

// Before the first tile: zero accumulators, pi's two LDS blocks, the tiles' constant columns (ends with a barrier), then the
// launch's scalars.
template <int D, int H, int A>
__device__ __forceinline__ void sac_prologue(SacNet<D, H, A>& net, const SacActorArgs& a, float* sm, float* sl, float* xs, float* hs, float* qs,
                                             int lane, float& alpha, bool& any_reg, float (&nominal)[A], double (&st)[SacLayout<D, H, A>::NS]) {
  using Net = PpoNet<D, H, A>;
  constexpr int XS = Net::XS, HS = Net::HS;
  net.zero();
  {
    PpoArgs p{};
    p.w = a.w;
    p.noise = a.noise;
    Net::fill(sm, p, lane);
    SacNet<D, H, A>::fill(sl, a.w, lane);
  }
  for (int i = lane; i < 64 * XS; i += 64) xs[i] = (i % XS == D) ? 1.0f : 0.0f;  // the ones column; the rest of the padding stays zero
  for (int i = lane; i < 64 * HS; i += 64) hs[i] = (i % HS == H) ? 1.0f : 0.0f;
  for (int i = lane; i < 64 * kMgX; i += 64) qs[i] = 0.0f;                       // columns past the critics' row stay zero
  __syncthreads();
  alpha = a.alpha_dev ? a.alpha_dev[0] : a.alpha;
  any_reg = a.lam_T != 0.0f || a.lam_S != 0.0f || a.lam_M != 0.0f;
#pragma unroll
  for (int j = 0; j < A; ++j) nominal[j] = a.nominal ? a.nominal[j] : 0.0f;
#pragma unroll
  for (int q = 0; q < SacLayout<D, H, A>::NS; ++q) st[q] = 0.0;
}

// The replay-buffer row of minibatch position pos: never a read outside the buffer
__device__ __forceinline__ int64_t sac_row_index(const int64_t* index, int64_t rows, int64_t pos, bool active) {
  const int64_t i = active ? (index ? index[pos] : pos) : 0;
  return i < 0 ? 0 : (i >= rows ? rows - 1 : i);
}

// One row of a draw, by minibatch position; NULL: zeros through the same code
template <int A>
__device__ __forceinline__ void sac_noise_row(const float* p, int64_t pos, bool active, float (&e)[A]) {
#pragma unroll
  for (int j = 0; j < A; ++j) e[j] = (p && active) ? p[pos * A + j] : 0.0f;
}

// The critics' phase: for Q1 then Q2, refill the critic's LDS arrays and the resident fc2_w, then Q and dQ/da of the rows in qs per
// half tile into dq[n].  IN: the critics' row width; acol: agent k's action columns in it.  Starts and ends with a barrier.
template <int A>
__device__ __forceinline__ void sac_critics(const MlpNetW (&q)[2], int IN, int acol, int QH, const float* qs, float* w1s, float* w2ts,
                                            float* svec, float* was, float* dq, int lane) {
#pragma unroll 1
  for (int n = 0; n < 2; ++n) {
    __syncthreads();  // the previous critic's reads are done
    float a2[4][4][4];
    {
      float a2t[4][4][4];
      load_fc2(a2, a2t, q[n].fc2_w, QH, lane);
#pragma unroll
      for (int k = 0; k < 64; ++k) w2ts[64 * k + lane] = a2t[k >> 4][(k >> 2) & 3][k & 3];
    }
    twinq_fill_small(w1s, svec, q[n], IN, QH, lane);
#pragma unroll
    for (int j = 0; j < 4; ++j) was[4 * lane + j] = (lane < QH && j < A) ? q[n].fc1_w[lane * IN + acol + j] : 0.0f;
    const float bias3 = q[n].fc3_b[0];
    __syncthreads();
#pragma unroll 1
    for (int half = 0; half < 2; ++half)
      dpg_q1_half<A>(a2, lds_here(w2ts), qs + 32 * half * kMgX, lds_here(w1s), lds_here(svec), was, dq + (n * 64 + 32 * half) * kDpgQ, bias3, lane);
  }
  __syncthreads();
}

// min(Q1, Q2): a row's gradient goes to the smaller critic; torch gives each half on an exact tie.  ga = d(-mean min Q) / da
template <int A, int NS>
__device__ __forceinline__ void sac_select(const float* dq, float inv_b, bool active, int lane, double (&st)[NS], float (&ga)[A]) {
  const float* dq1 = dq + 64 * kDpgQ;
  const float q1 = dq[lane * kDpgQ + 4], q2 = dq1[lane * kDpgQ + 4];
  const float w2 = q2 < q1 ? 1.0f : (q2 == q1 ? 0.5f : 0.0f);
  if (active) {
    st[0] += (double)fminf(q1, q2);
    st[6] += q2 < q1 ? 1.0 : 0.0;
  }
#pragma unroll
  for (int j = 0; j < A; ++j) {
    const float d1 = dq[lane * kDpgQ + j], d2 = dq1[lane * kDpgQ + j];
    const float d = w2 == 1.0f ? d2 : (w2 == 0.0f ? d1 : 0.5f * d1 + 0.5f * d2);
    ga[j] = -inv_b * d;
  }
}

// policy_regularization: its own sample r on the tile's rows (in xs) and the three smoothness terms.  i: the lane's replay-buffer
// row, pos: its minibatch position; xs is restored from columns [xcol, xcol + D) of qs.  Ends with a barrier.
template <int D, int H, int A>
__device__ __forceinline__ void sac_regularize(SacNet<D, H, A>& net, const SacActorArgs& a, const float* sm, const float* sl, float* xs, float* hs,
                                               float* ds, const float* qs, const float** src, int xcol, const float (&nominal)[A],
                                               double (&st)[SacLayout<D, H, A>::NS], int64_t i, int64_t pos, bool active, int lane) {
  using Net = PpoNet<D, H, A>;
  using SN = SacNet<D, H, A>;
  constexpr int XS = Net::XS;
  float x[D], h1[H], h2[H], mean[A], lsr[A], e[A], r[A], gr[A];
#pragma unroll
  for (int k = 0; k < D; ++k) x[k] = xs[lane * XS + k];
  SN::forward(sm, sl, x, h1, h2, mean, lsr);
  sac_noise_row(a.eps[1], pos, active, e);
  SacRow<A> s;
  s.sample(mean, lsr, e);
#pragma unroll
  for (int j = 0; j < A; ++j) {
    r[j] = fminf(fmaxf(s.act[j], -a.max_action), a.max_action);
    gr[j] = 0.0f;
  }
  if (a.lam_M != 0.0f) {
#pragma unroll
    for (int j = 0; j < A; ++j) {
      const float d = r[j] - nominal[j];
      if (active) st[4] += (double)(d * d);
      gr[j] = fmaf(a.c_M, d, gr[j]);
    }
  }
  // a smoothness pass on other input rows y: the difference enters both ends — gr for r's pass, -c d for y's own, here
  auto other = [&](const float (&y)[D], int which, float c, double& sum) {
    float g1[H], g2[H], mo[A], lo[A], eo[A], go[A], dmo[A], dlo[A];
    SN::forward(sm, sl, y, g1, g2, mo, lo);
    sac_noise_row(a.eps[which], pos, active, eo);
    SacRow<A> so;
    so.sample(mo, lo, eo);
#pragma unroll
    for (int j = 0; j < A; ++j) {
      const float d = r[j] - fminf(fmaxf(so.act[j], -a.max_action), a.max_action);
      if (active) sum += (double)(d * d);
      gr[j] = fmaf(c, d, gr[j]);
      go[j] = fabsf(so.act[j]) <= a.max_action ? -c * d : 0.0f;
    }
    so.deltas(go, 0.0f, active, dmo, dlo);
    net.backward(sm, sl, xs, hs, ds, g1, g2, dmo, dlo, lane);
  };
  if (a.lam_S != 0.0f) {
    float y[D];
#pragma unroll
    for (int k = 0; k < D; ++k) { y[k] = xs[lane * XS + k] + sm[Net::O_NOISE + k]; xs[lane * XS + k] = y[k]; }
    other(y, 3, a.c_S, st[3]);
  }
  if (a.lam_T != 0.0f) {
    src[lane] = active ? a.obs_next + i * D : nullptr;
    __syncthreads();
    ppo_stage<D, XS>(xs, src, lane);
    __syncthreads();
    float y[D];
#pragma unroll
    for (int k = 0; k < D; ++k) y[k] = xs[lane * XS + k];
    other(y, 2, a.c_T, st[2]);
  }
  if (a.lam_S != 0.0f || a.lam_T != 0.0f) {
#pragma unroll
    for (int k = 0; k < D; ++k) xs[lane * XS + k] = qs[lane * kMgX + xcol + k];
  }
  float ga[A], dmean[A], dls[A];
#pragma unroll
  for (int j = 0; j < A; ++j) ga[j] = fabsf(s.act[j]) <= a.max_action ? gr[j] : 0.0f;
  s.deltas(ga, 0.0f, active, dmean, dls);
  net.backward(sm, sl, xs, hs, ds, h1, h2, dmean, dls, lane);  // (ends with a barrier: the tiles are free for the next rows)
}

// After the last tile: the workgroup's ONE partial vector P — the eight tensors' accumulators, then the per-lane sums added across
// the lanes in lane order through red (64 x NS doubles of LDS that nothing else reads any more).
template <int D, int H, int A>
__device__ __forceinline__ void sac_epilogue(const SacNet<D, H, A>& net, double* P, double* red, const double (&st)[SacLayout<D, H, A>::NS], int lane) {
  using Net = PpoNet<D, H, A>;
  using PY = PpoLayout<D, H, A>;
  using Y = SacLayout<D, H, A>;
  Net::template emit<D, Net::NB1>(P + PY::O_W1, P + PY::O_B1, net.acc1, H, lane);
  Net::template emit<H, Net::NBH>(P + PY::O_W2, P + PY::O_B2, net.acc2, H, lane);
  Net::template emit<H, Net::NBH>(P + PY::O_W3, P + PY::O_B3, net.acc3, A, lane);
  SacNet<D, H, A>::emit_head2(P + Y::O_LW, P + Y::O_LB, net.acc3, lane);
  __syncthreads();
#pragma unroll
  for (int q = 0; q < Y::NS; ++q) red[lane * Y::NS + q] = st[q];
  __syncthreads();
  if (lane < Y::NS) {
    double s = 0.0;
    for (int l = 0; l < 64; ++l) s += red[l * Y::NS + lane];
    P[Y::O_ST + lane] = s;
  }
}

// One wavefront per workgroup owns 64-row tiles of the minibatch and walks them grid-stride.  Per tile, in this order:
//   the loss pass   gather the obs rows (index) through the LDS tile, forward (lane = row), sample with eps[0]; [obs | a] into the
//                   critic's tile; for Q1 then Q2: refill the critic's LDS arrays and the resident fc2_w, then Q and dQ/da per half
//                   tile on the matrix cores (dpg_q1_half); back on lane = row the selection, the deltas, one backward pass;
//   (any lam != 0)  the regulariser's own sample r on the same rows (eps[1]), forward only;
//   (lam_S != 0)    forward and backward on obs + noise (eps[3]);   (lam_T != 0)  the same on obs_next (eps[2]);
//                   r's backward pass with the differences of all three terms.
// Every pass adds into the same resident accumulators.  At the end the workgroup writes ONE partial vector.
template <int D, int H, int A>
__global__ __launch_bounds__(64) void sac_actor_kernel(const SacActorArgs a) {
  using Net = PpoNet<D, H, A>;
  using SN = SacNet<D, H, A>;
  using Y = SacLayout<D, H, A>;
  constexpr int XS = Net::XS, HS = Net::HS;
  __shared__ float sm[Net::SM], sl[SN::SL];
  __shared__ float xs[64 * XS], hs[64 * HS], ds[64 * kPpoDelta];
  __shared__ __attribute__((aligned(8))) float qs[64 * kMgX];  // the critics' input tile; at the end: the lanes' sums (float64)
  __shared__ float w1s[TwinQL1::SIZE], w2ts[64 * 64], svec[kTqVec], was[64 * 4], dq[2][64 * kDpgQ];
  __shared__ const float* src[64];
  static_assert(64 * Y::NS * sizeof(double) <= sizeof(float) * 64 * kMgX, "the sums fit the critics' tile");
  const int lane = threadIdx.x;
  SN net;
  float alpha, nominal[A];
  bool any_reg;
  double st[Y::NS];
  sac_prologue(net, a, sm, sl, xs, hs, qs, lane, alpha, any_reg, nominal, st);

  const int64_t tiles = (a.B + 63) / 64;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t row0 = tile * 64;
    const bool active = row0 + lane < a.B;
    const int64_t i = sac_row_index(a.index, a.rows, row0 + lane, active);
    src[lane] = active ? a.obs + i * D : nullptr;
    __syncthreads();
    ppo_stage<D, XS>(xs, src, lane);
    __syncthreads();

    // ---- the loss pass
    {
      float x[D], h1[H], h2[H], mean[A], lsr[A], e[A];
#pragma unroll
      for (int k = 0; k < D; ++k) x[k] = xs[lane * XS + k];
      SN::forward(sm, sl, x, h1, h2, mean, lsr);
      sac_noise_row(a.eps[0], row0 + lane, active, e);
      SacRow<A> s;
      s.sample(mean, lsr, e);
      if (active) {
        st[1] += (double)s.logp;
#pragma unroll
        for (int j = 0; j < A; ++j) st[5] += s.in[j] ? 0.0 : 1.0;
      }
      // the critics' phase needs the registers: x waits in its tile (and in qs), pi's activations in the two tiles that are free
      // until the backward pass
#pragma unroll
      for (int k = 0; k < D; ++k) qs[lane * kMgX + k] = x[k];
#pragma unroll
      for (int u = 0; u < H; ++u) { hs[lane * HS + u] = h1[u]; ds[lane * kPpoDelta + u] = h2[u]; }
#pragma unroll
      for (int j = 0; j < A; ++j) qs[lane * kMgX + D + j] = s.act[j];  // no clamp on the loss pass's action
      sac_critics<A>(a.q, D + A, D, a.hidden, qs, w1s, w2ts, svec, was, dq[0], lane);
#pragma unroll
      for (int u = 0; u < H; ++u) { h1[u] = hs[lane * HS + u]; h2[u] = ds[lane * kPpoDelta + u]; }
      float ga[A], dmean[A], dls[A];
      sac_select(dq[0], a.inv_b, active, lane, st, ga);
      s.deltas(ga, alpha * a.inv_b, active, dmean, dls);
      net.backward(sm, sl, xs, hs, ds, h1, h2, dmean, dls, lane);  // (ends with a barrier)
    }

    if (any_reg) sac_regularize(net, a, sm, sl, xs, hs, ds, qs, src, 0, nominal, st, i, row0 + lane, active, lane);
  }

  sac_epilogue(net, a.partials + (int64_t)blockIdx.x * Y::NP, reinterpret_cast<double*>(qs), st, lane);
}

// Agent k of two under one centralized twin critic (qr_ctde_sac_actor_grad): <15, 16, 4> for k = 0, <3, 4, 1> for k = 1.
// sac_actor_kernel's walk in its two-agent form, as dpg_walk's CT form (qr_td3_actor.h).  The critics' tile takes the other
// agent's observation rows at their columns (stage_rows, a second pointer array) and its action: supplied by minibatch position, or
// pi_{1-k} forward only on the lane's own row from LDS (SacNet::forward of the pair's other size), sampled with eps_other, tanh, no
// clamp, before agent k's own pass so that it holds no register across the critics' phase.  Agent k's observation and action go to
// their own columns, `was` is fc1_w's columns of a_k, the critics' row is in_dim wide.  With eps_logp the reference's SECOND sample
// of pi_k carries the entropy term: it shares the loss pass's forward (same row, same mean and raw log_std), its deltas (ga = 0,
// gl = alpha / B) are formed right after it and wait in LDS (park) across the critics' phase, then add to the first sample's (whose
// gl is then 0) before the ONE backward pass; logp and alpha's gradient are the second sample's.  Without it: the one-agent arithmetic.
// The other agent's action is a VALUE: no gradient for agent 1-k is produced and nothing of that actor is written (the reference's
// backward pass leaves one in that actor's .grad, which that agent zeroes before anything reads it; include/quadrotor_hip.h).
// Shared with sac_actor_kernel: every block above.  This kernel's own: the other agent's staging and action, the second sample with
// its park tile, the choice of gl, and the glue of the loss pass, which differs in every other line (xcol, acol, `two`).  The walk as
// ONE force-inlined function, dpg_walk's way, cost the one-agent kernels 24 and 48 bytes of scratch per lane; block
// by block all five instantiations stay at or below their registers, LDS and scratch from before the blocks were shared.
template <int D, int H, int A>
__global__ __launch_bounds__(64) void ctde_sac_actor_kernel(const CtdeSacActorArgs a) {
  using Net = PpoNet<D, H, A>;
  using SN = SacNet<D, H, A>;
  using Y = SacLayout<D, H, A>;
  constexpr int XS = Net::XS, HS = Net::HS;
  __shared__ float sm[Net::SM], sl[SN::SL];
  __shared__ float xs[64 * XS], hs[64 * HS], ds[64 * kPpoDelta];
  __shared__ __attribute__((aligned(8))) float qs[64 * kMgX];  // the critics' input tile; at the end: the lanes' sums (float64)
  __shared__ float w1s[TwinQL1::SIZE], w2ts[64 * 64], svec[kTqVec], was[64 * 4], dq[2][64 * kDpgQ];
  __shared__ const float* src[64];
  static_assert(64 * Y::NS * sizeof(double) <= sizeof(float) * 64 * kMgX, "the sums fit the critics' tile");
  constexpr int OD = D == 15 ? 3 : 15, OH = D == 15 ? 4 : 16, OA = D == 15 ? 1 : 4;  // the Decoupled pair's other half
  using ONet = PpoNet<OD, OH, OA>;
  using OSN = SacNet<OD, OH, OA>;
  __shared__ const float* src1[64];
  __shared__ float osm[ONet::SM], osl[OSN::SL];
  __shared__ float park[2 * A * 64];  // the second sample's dmean, dls: [2 A][64 lanes]
  static_assert(sizeof(sm) + sizeof(sl) + sizeof(xs) + sizeof(hs) + sizeof(ds) + sizeof(qs) + sizeof(w1s) + sizeof(w2ts) + sizeof(svec) +
                        sizeof(was) + sizeof(dq) + sizeof(src) + sizeof(src1) + sizeof(osm) + sizeof(osl) + sizeof(park) <= 64 * 1024 - 64,
                "static LDS stays under 64 KB");
  const int lane = threadIdx.x;
  const int xcol = a.col_own, acol = a.acol_own;  // agent k's observation and action columns in the critics' row
  const bool two = a.eps_logp != nullptr;         // the entropy term comes from a second sample
  if (!a.action_other) {                          // (before the prologue's barrier)
    PpoArgs p{};
    p.w = a.other;
    ONet::fill(osm, p, lane);
    OSN::fill(osl, a.other, lane);
  }
  SN net;
  float alpha, nominal[A];
  bool any_reg;
  double st[Y::NS];
  sac_prologue(net, a, sm, sl, xs, hs, qs, lane, alpha, any_reg, nominal, st);

  const int64_t tiles = (a.B + 63) / 64;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t row0 = tile * 64;
    const bool active = row0 + lane < a.B;
    const int64_t i = sac_row_index(a.index, a.rows, row0 + lane, active);
    src[lane] = active ? a.obs + i * D : nullptr;
    src1[lane] = active ? a.obs_other + i * a.od_other : nullptr;
    __syncthreads();
    ppo_stage<D, XS>(xs, src, lane);
    stage_rows(qs, kMgX, src1, a.od_other, a.col_other, lane);
    __syncthreads();
    {  // the other agent's action: a value only
      float* qa = qs + lane * kMgX + a.acol_other;
      if (a.action_other) {
        for (int f = 0; f < a.ad_other; ++f) qa[f] = active ? a.action_other[(row0 + lane) * a.ad_other + f] : 0.0f;
      } else {
        float xo[OD], g1[OH], g2[OH], mo[OA], lo[OA], eo[OA];
#pragma unroll
        for (int k = 0; k < OD; ++k) xo[k] = qs[lane * kMgX + a.col_other + k];
        OSN::forward(osm, osl, xo, g1, g2, mo, lo);
#pragma unroll  // (not through sac_noise_row<OA>: that moved <3,4,1>'s scratch from 1504 to 1520 bytes per lane, the parent's being 1512)
        for (int f = 0; f < OA; ++f) eo[f] = (a.eps_other && active) ? a.eps_other[(row0 + lane) * OA + f] : 0.0f;
        SacRow<OA> so;
        so.sample(mo, lo, eo);
#pragma unroll
        for (int f = 0; f < OA; ++f) qa[f] = so.act[f];  // no clamp, as agent k's own
      }
    }

    // ---- the loss pass
    {
      float x[D], h1[H], h2[H], mean[A], lsr[A], e[A];
#pragma unroll
      for (int k = 0; k < D; ++k) x[k] = xs[lane * XS + k];
      SN::forward(sm, sl, x, h1, h2, mean, lsr);
      sac_noise_row(a.eps[0], row0 + lane, active, e);
      SacRow<A> s;
      s.sample(mean, lsr, e);
      if (active) {
        if (!two) st[1] += (double)s.logp;
#pragma unroll
        for (int j = 0; j < A; ++j) st[5] += s.in[j] ? 0.0 : 1.0;
      }
      if (two) {  // the second sample of the same forward pass: logp, and its deltas into LDS
        float e2[A], g0[A], dm2[A], dl2[A];
#pragma unroll
        for (int j = 0; j < A; ++j) { e2[j] = active ? a.eps_logp[(row0 + lane) * A + j] : 0.0f; g0[j] = 0.0f; }
        SacRow<A> s2;
        s2.sample(mean, lsr, e2);
        if (active) st[1] += (double)s2.logp;
        s2.deltas(g0, alpha * a.inv_b, active, dm2, dl2);
#pragma unroll
        for (int j = 0; j < A; ++j) { park[j * 64 + lane] = dm2[j]; park[(A + j) * 64 + lane] = dl2[j]; }
      }
      // the critics' phase needs the registers: x waits in its tile (and in qs), pi's activations in the two tiles that are free
      // until the backward pass
#pragma unroll
      for (int k = 0; k < D; ++k) qs[lane * kMgX + xcol + k] = x[k];
#pragma unroll
      for (int u = 0; u < H; ++u) { hs[lane * HS + u] = h1[u]; ds[lane * kPpoDelta + u] = h2[u]; }
#pragma unroll
      for (int j = 0; j < A; ++j) qs[lane * kMgX + acol + j] = s.act[j];  // no clamp on the loss pass's action
      sac_critics<A>(a.q, a.in_dim, acol, a.hidden, qs, w1s, w2ts, svec, was, dq[0], lane);
#pragma unroll
      for (int u = 0; u < H; ++u) { h1[u] = hs[lane * HS + u]; h2[u] = ds[lane * kPpoDelta + u]; }
      float ga[A], dmean[A], dls[A];
      sac_select(dq[0], a.inv_b, active, lane, st, ga);
      s.deltas(ga, two ? 0.0f : alpha * a.inv_b, active, dmean, dls);
      if (two) {
#pragma unroll
        for (int j = 0; j < A; ++j) { dmean[j] += park[j * 64 + lane]; dls[j] += park[(A + j) * 64 + lane]; }
      }
      net.backward(sm, sl, xs, hs, ds, h1, h2, dmean, dls, lane);  // (ends with a barrier)
    }

    if (any_reg) sac_regularize(net, a, sm, sl, xs, hs, ds, qs, src, xcol, nominal, st, i, row0 + lane, active, lane);
  }

  sac_epilogue(net, a.partials + (int64_t)blockIdx.x * Y::NP, reinterpret_cast<double*>(qs), st, lane);
}


struct SacActorReduceArgs {
  const double* partials;   // [n_parts][np]
  float* grad[8];           // fc1_w, fc1_b, fc2_w, fc2_b, mean_w, mean_b, log_std_w, log_std_b
  float* stats;             // [6]
  float* alpha_grad;        // one float or NULL
  const float* alpha_dev;   // device scalar, or NULL: `alpha`
  int32_t off[9];           // start of each gradient tensor in a partial vector; off[8] = the seven sums
  int32_t n_parts, np;
  double B, BA;             // rows, rows x action_dim
  float alpha, target_entropy, lam_T, lam_S, lam_M;
};

// Workgroups 0 .. gridDim.x - 2: sixteen consecutive gradient entries each (reduce16_entries).  The last one: the seven sums (256
// strided slices each, then a tree), and from them `stats` and alpha's gradient.
__global__ __launch_bounds__(256) void sac_actor_reduce_kernel(const SacActorReduceArgs o) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  if (blockIdx.x + 1 < gridDim.x) {
    const int e = reduce16_entries(o.partials, o.n_parts, o.np, o.off[8], red);
    if (e >= 0) {
      const int k = entry_tensor<8>(e, o.off);
      float* dst = o.grad[0];
#pragma unroll
      for (int j = 1; j < 8; ++j)
        if (k == j) dst = o.grad[j];
      dst[e - o.off[k]] = (float)red[t];
    }
    return;
  }
  double s[7];
#pragma unroll
  for (int q = 0; q < 7; ++q) s[q] = block_sum_column(o.partials + o.off[8] + q, o.n_parts, o.np, red);
  if (t == 0) {
    const double alpha = o.alpha_dev ? (double)o.alpha_dev[0] : (double)o.alpha;
    const double reg = ((double)o.lam_T * s[2] + (double)o.lam_S * s[3] + (double)o.lam_M * s[4]) / o.BA;
    o.stats[0] = (float)(alpha * s[1] / o.B - s[0] / o.B + reg);
    o.stats[1] = (float)(s[0] / o.B);
    o.stats[2] = (float)(s[1] / o.B);
    o.stats[3] = (float)reg;
    o.stats[4] = (float)(s[5] / o.BA);
    o.stats[5] = (float)(s[6] / o.B);
    if (o.alpha_grad) o.alpha_grad[0] = (float)(-((double)o.target_entropy + s[1] / o.B));
  }
}

}  // namespace qr
