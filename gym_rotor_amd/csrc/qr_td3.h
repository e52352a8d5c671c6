// qr_td3.h — part of the gfx950 quadrotor step library (included by quadrotor_kernels.hip after qr_optim.h, and by qr_td3_actor.h and qr_sac.h).
// The critic half of one TD3 minibatch update (TD3.train, algos/td3/td3.py:123-167, the non-CTDE branch) for the reference's twin
// critic MLP_Critic (algos/td3/td3_mlp.py:36-99; Q = fc3(relu(fc2(relu(fc1(sa))))), twice):
//   td3_target_kernel  (qr_twinq_target)   y = reward + discount (1 - done) min(Q1_targ, Q2_targ)(obs_next, a'), forward only:
//                                           target_walk with Td3Rule; the walk is sac_target_kernel's too (qr_sac.h)
//   twinq_kernel + twinq_reduce_kernel (qr_twinq_grad)   mse(Q1, y) + mse(Q2, y) and its gradients for the twelve tensors
// The tile walk, the half-tile body, the partial vector and the reduction's sums are qr_mlp_grad.h's, shared with ppo_critic_kernel; here, as
// TwinQL1 and TqRule: ReLU, 28 inputs with fc1_w's operands in LDS, rows from obs + action, y by minibatch position, two statistics, two networks.
// The centralized (CTDE) critic of two agents (td3.py:124-137, 157-158; sac.py:136-144, 156-157) is the same code on rows from four
// sources: ctde_twinq_kernel (qr_ctde_twinq_grad) and target_walk's two-agent forms (qr_ctde_twinq_target, qr_ctde_sac_target).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "quadrotor_hip.h"
#include "qr_actor.h"
#include "qr_mlp_grad.h"

namespace qr {

struct TwinQArgs {
  MlpNetW net[2];                    // workgroup row blockIdx.y owns net[blockIdx.y]
  const float* obs;                  // [>= rows][obs_dim]
  const float* action;               // row i at action + i * act_stride (the column offset is already added)
  const float* y;                    // [B], by minibatch position
  const int64_t* index;              // [B] or NULL (rows 0..B-1)
  double* partials;                  // [2][grid][np]
  int64_t B, rows;
  int32_t obs_dim, action_dim, hidden, act_stride;
  float g_scale;                     // 2 / B: dLoss / dQ = g_scale * e
};

constexpr int kTqSums = 2;  // the statistics behind one network's gradients in a partial vector: sum e^2, sum y

// mlp_grad_half's traits: ReLU — the activation t = max(z, 0) is what is stored, and the delta through it is d * (t > 0); 28 inputs
// (obs_dim + action_dim: the Coupled critic has 23 + 4; 7 k-steps), the ones in column 28; fc1_w in LDS as layer 1's A operands in
// the lane map: entry (hb, s) of lane l at [(hb * KS + s) * 64 + l].  Read per k-step and not kept resident: the seventh k-step of
// the 28-wide input would need 4 registers the gradient kernel does not have, and the 28 reads per half tile (conflict-free, one
// dword per lane) ride under 56 MFMAs.
struct TwinQL1 {
  static constexpr int KS = 7, ONES = 28, XS = 28, SIZE = 4 * KS * 64;
  const float* w1;  // behind lds_here

  static __device__ __forceinline__ float act(float z) { return fmaxf(z, 0.0f); }
  static __device__ __forceinline__ float dact(float t, float d) { return t > 0.0f ? d : 0.0f; }
  __device__ __forceinline__ float a1(int hb, int s, int lane) const { return w1[(hb * KS + s) * 64 + lane]; }
};

constexpr int kTqVec = kMgB3 + 4;  // the small vectors, then fc3_b

__device__ __forceinline__ void twinq_fill_small(float* w1s, float* svec, const MlpNetW& p, int D, int H, int lane) {
  const int c = lane & 15, g = lane >> 4;
#pragma unroll
  for (int hb = 0; hb < 4; ++hb) {
    const int row = 16 * hb + c;
#pragma unroll
    for (int s = 0; s < TwinQL1::KS; ++s)
      w1s[(hb * TwinQL1::KS + s) * 64 + lane] = (row < H && 4 * s + g < D) ? p.fc1_w[row * D + 4 * s + g] : 0.0f;
  }
  fill_vecs(svec, p, H, lane);
  if (lane == 0) svec[kMgB3] = p.fc3_b[0];
}

// mlp_grad_walk's rule (qr_mlp_grad.h): workgroup row blockIdx.y owns net[blockIdx.y]; the observation row, then the action row, both
// always staged; fc1_w's operands and fc3_b in LDS, read behind lds_here per half tile; y by minibatch position; two statistics.
struct TqRule {
  using Args = TwinQArgs;
  using L1 = TwinQL1;
  static constexpr int SUMS = kTqSums, W1S = TwinQL1::SIZE, SVEC = kTqVec;
  static constexpr int SRC = 2;
  static constexpr bool SKIP_EMPTY = false;
  static __device__ __forceinline__ int width(const Args& a, int s) { return s ? a.action_dim : a.obs_dim; }
  static __device__ __forceinline__ const MlpNetW& net(const Args& a) { return blockIdx.y ? a.net[1] : a.net[0]; }
  __device__ __forceinline__ void fill(float* w1s, float* svec, const MlpNetW& w, int D, int H, int lane) { twinq_fill_small(w1s, svec, w, D, H, lane); }
  __device__ __forceinline__ L1 layer1(const float* w1s) const { return L1{lds_here(w1s)}; }
  static __device__ __forceinline__ const float* row(const Args& a, int64_t i, int s) { return s ? a.action + i * a.act_stride : a.obs + i * a.obs_dim; }
  static __device__ __forceinline__ float target(const Args& a, int64_t, int64_t j) { return a.y[j]; }
  static __device__ __forceinline__ void stat(double (&st)[SUMS], float e, float y) { st[0] += (double)e * (double)e; st[1] += (double)y; }
};

__global__ __launch_bounds__(64) void twinq_kernel(const TwinQArgs a) { mlp_grad_walk<TqRule>(a); }

// The centralized (CTDE) twin critic of two agents, MLP_Critic_CTDE (td3_mlp.py:102-168): the same regression on the row
// [obs_0 | obs_1 | act_0 | act_1], formed in the walk's tile from its four sources (qr_ctde_twinq_grad).  Everything behind the
// staging is TqRule's, so the partial vector and twinq_reduce_kernel serve as they are.
struct CtdeTwinQArgs {
  MlpNetW net[2];
  const float* obs[2];               // [>= rows][obs_dim[m]]
  const float* action[2];            // row i of agent m at action[m] + i * act_stride[m] (the column offset is already added)
  const float* y;
  const int64_t* index;
  double* partials;
  int64_t B, rows;
  int32_t obs_dim[2], action_dim[2], act_stride[2], hidden;
  float g_scale;
};

struct CtdeTqRule : TqRule {
  using Args = CtdeTwinQArgs;
  static constexpr int SRC = 4;
  static __device__ __forceinline__ int width(const Args& a, int s) { return s < 2 ? a.obs_dim[s] : a.action_dim[s - 2]; }
  static __device__ __forceinline__ const MlpNetW& net(const Args& a) { return blockIdx.y ? a.net[1] : a.net[0]; }
  static __device__ __forceinline__ const float* row(const Args& a, int64_t i, int s) {
    return s < 2 ? a.obs[s] + i * a.obs_dim[s] : a.action[s - 2] + i * a.act_stride[s - 2];
  }
  static __device__ __forceinline__ float target(const Args& a, int64_t, int64_t j) { return a.y[j]; }
};

__global__ __launch_bounds__(64) void ctde_twinq_kernel(const CtdeTwinQArgs a) { mlp_grad_walk<CtdeTqRule>(a); }

struct TwinQReduceArgs {
  const double* partials;   // [2][n_parts][np]
  float* grad[2][6];        // per network: fc1_w, fc1_b, fc2_w, fc2_b, fc3_w, fc3_b
  float* stats;             // [4]
  int32_t off[7];           // start of each gradient tensor in a partial vector; off[6] = the two sums
  int32_t n_parts, np;
  double B;
};

// Workgroup row blockIdx.y: one network.  Workgroups 0 .. gridDim.x - 2 of a row: sixteen consecutive gradient entries each of the
// network's partial vectors (reduce16_entries).  The last workgroup of row 0: the sums of both networks (256 strided slices each,
// then a tree), and from them `stats`.
__global__ __launch_bounds__(256) void twinq_reduce_kernel(const TwinQReduceArgs o) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  const int nn = blockIdx.y;
  const double* net1 = o.partials + (int64_t)o.n_parts * o.np;
  if (blockIdx.x + 1 < gridDim.x) {
    reduce16_store(nn ? net1 : o.partials, o.n_parts, o.np, o.off, nn ? o.grad[1] : o.grad[0], red, [](int, int, double v) { return v; });
    return;
  }
  if (nn) return;
  const double* col[3] = {o.partials + o.off[6], o.partials + o.off[6] + 1, net1 + o.off[6]};  // sum e1^2, sum y, sum e2^2
  double sums[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) sums[q] = block_sum_column(col[q], o.n_parts, o.np, red);
  if (t == 0) {
    const double m1 = sums[0] / o.B, m2 = sums[2] / o.B;
    o.stats[0] = (float)(m1 + m2);
    o.stats[1] = (float)m1;
    o.stats[2] = (float)m2;
    o.stats[3] = (float)(sums[1] / o.B);
  }
}

// ------------------------------------------------------------------------------------------------------------------
// qr_twinq_target, qr_ctde_twinq_target
// ------------------------------------------------------------------------------------------------------------------
// Per-agent members are arrays of two: the one-agent entry fills [0] and its kernels never read [1]; the centralized (CTDE) entries
// (quadrotor_kernels.hip) fill both, and `own` = the agent whose reward and done columns these are.
struct Td3TargetArgs {
  ActorW actor[2];                   // pi_targ (AD > 0); log_std and the log_std head are NULL: never read
  MlpNetW net[2];                    // Q1_targ, Q2_targ
  const float* obs_next[2];          // [>= rows][obs_dim[m]]
  const float *reward, *done;        // element i at [i * rwd_stride] / [i * done_stride]
  const float* eps[2];               // [B][action_dim[m]] by minibatch position, or NULL
  const float* action_next[2];       // AD = 0: a' [B][action_dim[m]] by minibatch position, used as it is
  const int64_t* index;
  float* y;                          // [B]
  int64_t B, rows;
  int32_t obs_dim[2], action_dim[2], hidden, rwd_stride, done_stride, own;
  float discount, target_noise, noise_clip, max_action;
};

// One target network, forward only, over a whole tile: mlp_grad_half's forward pieces (qr_mlp_grad.h) with TwinQL1 — ReLU, seven
// k-steps, fc1's operands and the small vectors in LDS — and fc2_w resident (a2, load_fc2).
// xs: the tile [64 rows][kMgX]; returns Q of row `lane`
__device__ __forceinline__ float twinq_forward(const float (&a2)[4][4][4], const float* xs, const float* w1, const float* sv, int lane) {
  const int g = lane >> 4;
  float P[4];
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    f32x4 h1[4][2], h2[4][2];
    mlp_bias(h1, h2, sv, lane);
    mlp_layer1(h1, TwinQL1{w1}, xs + 32 * half * kMgX, lane);
#pragma unroll
    for (int hb = 0; hb < 4; ++hb) {
#pragma unroll
      for (int r = 0; r < 4; ++r) { h1[hb][0][r] = TwinQL1::act(h1[hb][0][r]); h1[hb][1][r] = TwinQL1::act(h1[hb][1][r]); }
    }
    mlp_layer2(h2, a2, h1);
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      float q[4];
#pragma unroll
      for (int ho = 0; ho < 4; ++ho) {
        q[ho] = sv[kMgW3 + 16 * ho + 4 * g] * TwinQL1::act(h2[ho][b][0]);
#pragma unroll
        for (int r = 1; r < 4; ++r) q[ho] = fmaf(sv[kMgW3 + 16 * ho + 4 * g + r], TwinQL1::act(h2[ho][b][r]), q[ho]);
      }
      P[2 * half + b] = (q[0] + q[1]) + (q[2] + q[3]);
    }
  }
  // P[b] of lane (g, c) = row 16 b + c's sum over hidden group g; the sum over g and the move of block b's result to lane row
  // g' = b (CriticMfma::forward)
  const auto s01 = __builtin_amdgcn_permlane16_swap(__float_as_uint(P[0]), __float_as_uint(P[1]), false, false);
  const auto s23 = __builtin_amdgcn_permlane16_swap(__float_as_uint(P[2]), __float_as_uint(P[3]), false, false);
  const float q01 = __uint_as_float(s01[0]) + __uint_as_float(s01[1]);
  const float q23 = __uint_as_float(s23[0]) + __uint_as_float(s23[1]);
  const auto t = __builtin_amdgcn_permlane32_swap(__float_as_uint(q01), __float_as_uint(q23), false, false);
  return sv[kMgB3] + (__uint_as_float(t[0]) + __uint_as_float(t[1]));
}

// What td3_target_kernel and sac_target_kernel (qr_sac.h) share: the tile walk.  AD = the actor's obs_dim: 23 or 15 (ActorMfma,
// hidden 16, 4 actions), 3 (ActorLds<3, 4, 1>), or 0: no actor, a' is supplied.  AD1 < 0: one agent.  AD1 >= 0: the centralized
// (CTDE) critic of two agents, whose row is [obs_next_0 | obs_next_1 | a'_0 | a'_1] — AD = 15 with AD1 = 3, both Decoupled actors in
// the one wave (agent 0's on the matrix cores with its weights resident, agent 1's from LDS), or AD = AD1 = 0, both a' supplied.
// One wavefront per workgroup walks 64-row tiles grid-stride: gather obs_next rows (index, clamped) into the critic's input tile and
// the actors' tiles, the actors' heads for the lane's own row, a' into the columns behind the observations, then both target
// networks over the tile and min.  Lane l owns row l.
// A Rule supplies what is the algorithm's own: Args (the fields read here carry the same names in both), LOG_STD (has the actor a
// log_std head), and for minibatch position j, with `sum` what the rule adds up over a row (zero at the row's start), m the agent,
// TWO = the centralized form and own = is m the agent whose row sum this is (always, with one agent):
//   component<TWO>(m, pre, ls, k, active, own, sum)  a' of one component from the heads' outputs; k = j * action_dim[m] + f
//   keep(m, k, act, active)                          a' of one component is settled, computed or supplied
//   supplied(j, active)                              `sum` of a row whose a' is supplied
//   bellman(j, rwd, dn, qmin, sum)                   y[j], for active rows only
template <int AD, class Rule, int AD1 = -1>
__device__ __forceinline__ void target_walk(const typename Rule::Args& a) {
  constexpr bool TWO = AD1 >= 0;
  static_assert(!TWO || (AD == 15 && AD1 == 3) || (AD == 0 && AD1 == 0), "the centralized form: both Decoupled actors or none");
  constexpr int AA = AD == 3 ? 1 : 4;  // the actor's action_dim
  using Actor1 = ActorLds<3, 4, 1>;
  constexpr bool LDS_ACTOR = AD == 3 || AD1 == 3;
  __shared__ float xs[64 * kMgX];
  __shared__ float as[AD > 0 ? 64 * AD : 4];
  __shared__ float as1[AD1 > 0 ? 64 * AD1 : 4];
  __shared__ __attribute__((aligned(16))) float wsm[LDS_ACTOR ? Actor1::SIZE : 4];
  __shared__ float w1s[2][TwinQL1::SIZE], svec[2][kTqVec];
  __shared__ const float* src0[64];
  __shared__ const float* src1[TWO ? 64 : 1];
  const int lane = threadIdx.x;
  const int od1 = TWO ? a.obs_dim[1] : 0, ad1 = TWO ? a.action_dim[1] : 0;
  const int OD = a.obs_dim[0] + od1;  // the observations' columns; a' behind them
  const int D = OD + a.action_dim[0] + ad1, H = a.hidden;
  float q1[4][4][4], q2[4][4][4];  // fc2_w of Q1_targ, Q2_targ
  load_fc2(q1, a.net[0].fc2_w, H, lane);
  load_fc2(q2, a.net[1].fc2_w, H, lane);
  twinq_fill_small(w1s[0], svec[0], a.net[0], D, H, lane);
  twinq_fill_small(w1s[1], svec[1], a.net[1], D, H, lane);
  ActorMfma<(AD == 23 || AD == 15) ? AD : 23, Rule::LOG_STD> actor;
  if constexpr (AD == 23 || AD == 15) actor.load(a.actor[0], lane);
  if constexpr (LDS_ACTOR) Actor1::fill(wsm, a.actor[AD == 3 ? 0 : 1], lane);
  const Rule rule(a);
  for (int i = lane; i < 64 * kMgX; i += 64) xs[i] = 0.0f;  // the padding columns stay zero: nothing below writes them
  __syncthreads();

  const int64_t tiles = (a.B + 63) / 64;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t row0 = tile * 64, j = row0 + lane;
    const bool active = j < a.B;
    int64_t i = active ? (a.index ? a.index[j] : j) : 0;
    i = i < 0 ? 0 : (i >= a.rows ? a.rows - 1 : i);  // never a read outside the buffer
    src0[lane] = active ? a.obs_next[0] + i * a.obs_dim[0] : nullptr;
    if constexpr (TWO) src1[lane] = active ? a.obs_next[1] + i * od1 : nullptr;
    const float rwd = active ? a.reward[i * a.rwd_stride] : 0.0f;
    const float dn = active ? a.done[i * a.done_stride] : 0.0f;
    __syncthreads();
    stage_rows(xs, kMgX, src0, a.obs_dim[0], 0, lane);
    if constexpr (TWO) stage_rows(xs, kMgX, src1, od1, a.obs_dim[0], lane);
    if constexpr (AD > 0) stage_rows(as, AD, src0, AD, 0, lane);
    if constexpr (AD1 > 0) stage_rows(as1, AD1, src1, AD1, 0, lane);
    __syncthreads();
    float sum = 0.0f;
    if constexpr (AD > 0) {
      const int acol = TWO ? OD : AD;
      float pre[AA], ls[AA];
      if constexpr (AD == 3) {
        float x[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) x[k] = as[lane * 3 + k];
        Actor1::heads(wsm, Rule::LOG_STD, x, pre, ls);
      } else {
        actor.heads(as, lane, pre, ls);
      }
      const bool own0 = !TWO || a.own == 0;
#pragma unroll
      for (int f = 0; f < AA; ++f) {
        const float act = rule.template component<TWO>(0, pre[f], ls[f], j * AA + f, active, own0, sum);
        xs[lane * kMgX + acol + f] = act;
        rule.keep(0, j * AA + f, act, active);
      }
      if constexpr (AD1 == 3) {
        float x[3], pre1[1], ls1[1];
#pragma unroll
        for (int k = 0; k < 3; ++k) x[k] = as1[lane * 3 + k];
        Actor1::heads(wsm, Rule::LOG_STD, x, pre1, ls1);
        const float act = rule.template component<TWO>(1, pre1[0], ls1[0], j, active, a.own == 1, sum);
        xs[lane * kMgX + acol + AA] = act;
        rule.keep(1, j, act, active);
      }
    } else {
      int col = OD;
#pragma unroll
      for (int m = 0; m < (TWO ? 2 : 1); ++m) {
        const int w = a.action_dim[m];
        for (int f = 0; f < w; ++f) {
          const float act = active ? a.action_next[m][j * w + f] : 0.0f;
          xs[lane * kMgX + col + f] = act;
          rule.keep(m, j * w + f, act, active);
        }
        col += w;
      }
      sum = rule.supplied(j, active);
    }
    __syncthreads();
    const float v1 = twinq_forward(q1, xs, lds_here(w1s[0]), lds_here(svec[0]), lane);
    const float v2 = twinq_forward(q2, xs, lds_here(w1s[1]), lds_here(svec[1]), lane);
    __syncthreads();  // the tile is read: the next one may be staged
    if (active) rule.bellman(j, rwd, dn, fminf(v1, v2), sum);
  }
}

// TD3's rule: the target actor's mean, the smoothing noise and both clamps; the Bellman line on min.
struct Td3Rule {
  using Args = Td3TargetArgs;
  static constexpr bool LOG_STD = false;
  const Args& a;
  __device__ __forceinline__ explicit Td3Rule(const Args& args) : a(args) {}
  template <bool TWO>
  __device__ __forceinline__ float component(int m, float pre, float, int64_t k, bool active, bool, float&) const {
    const float* eps = (TWO && m) ? a.eps[1] : a.eps[0];
    float n = 0.0f;
    if (eps && active) n = fminf(fmaxf(a.target_noise * eps[k], -a.noise_clip), a.noise_clip);
    return fminf(fmaxf(tanh_fast(pre) + n, -a.max_action), a.max_action);
  }
  __device__ __forceinline__ void keep(int, int64_t, float, bool) const {}
  __device__ __forceinline__ float supplied(int64_t, bool) const { return 0.0f; }
  __device__ __forceinline__ void bellman(int64_t j, float rwd, float dn, float qmin, float) const {
    a.y[j] = fmaf(a.discount * (1.0f - dn), qmin, rwd);
  }
};

template <int AD, int AD1 = -1>
__global__ __launch_bounds__(64) void td3_target_kernel(const Td3TargetArgs a) { target_walk<AD, Td3Rule, AD1>(a); }

}  // namespace qr
