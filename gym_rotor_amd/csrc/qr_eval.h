// qr_eval.h — part of the gfx950 quadrotor step library (included by quadrotor_kernels.hip, in this order).
// Batched policy evaluation (qr_evaluate_actor): the reference's Learner.eval_policy (main.py:270-404) for every env in one launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "quadrotor_hip.h"
#include "qr_actor.h"

namespace qr {

// What qr_evaluate_actor writes besides the env's own buffers and the final observation rows (Args::obs0 / obs1) and last
// actions (Args::act_out, optional).  Its own kernarg block behind Args: the step kernel's argument layout is untouched.
struct EvalArgs {
  double* ret;          // [N][NAG] sum of the rewards up to and including the terminal step
  double* bench;        // [N]      sum of benchmark_reward_func(ex, eb1) (utils/utils.py:42-47)
  int32_t* length;      // [N]      steps taken
  uint8_t* terminated;  // [N]      1 = ended by some agent's done flag
  uint8_t* success;     // [N][NAG] main.py:366-373 (length == max_steps and |ex|_inf <= 0.01; MODUL agent 1: |eb1| <= 0.01)
  float* final_error;   // [N][4]   ex, eb1 of the last step; may be NULL
  int32_t max_steps;
  // qr_evaluate_population: the env batch is P blocks of tiles_per_policy 64-env tiles, one policy each, of which the first
  // envs_per_policy envs are flown.  qr_evaluate_actor is P = 1: the host fills in N and the whole grid (do_evaluate).
  int32_t envs_per_policy;
  int32_t tiles_per_policy;
};
struct EvalLaunch {
  Args a;
  EvalArgs e;
};

// Policy p's copy of an actor whose tensors are stacked [P][...] (contiguous; the pointers are policy 0's): every tensor starts
// p * numel elements later.  The log_std sources stay as the host left them for an evaluation: cleared, never read.
template <int D, int H, int A>
__device__ __forceinline__ ActorW actor_of_policy(const ActorW& w, unsigned p) {
  ActorW o = w;
  o.fc1_w += p * unsigned(H * D); o.fc1_b += p * unsigned(H);
  o.fc2_w += p * unsigned(H * H); o.fc2_b += p * unsigned(H);
  o.mean_w += p * unsigned(A * H); o.mean_b += p * unsigned(A);
  return o;
}

// One lane = one env, one 64-lane wave = one tile, as in step_kernel's POLICY path without a helper wave — and with its arithmetic:
// the deterministic action of the actor(s) on the current observation (MFMA actor; Decoupled agent 1 per lane from LDS), the fused
// goal generator (TRAJ as in step_kernel), action map, `substeps` plain substeps (RK4, or Magnus when MAG), error observation, reward,
// done and the crash override, then pack / unpack of the attitude as every multi-step launch does between env-steps.  No per-step
// row is written and nothing is ever re-sampled.  A lane FREEZES at the first step that sets any agent's done flag (or at max_steps):
// it writes its state, integrators, generator state, final rows and results back right there, once, and its registers are dead from
// then on.  A tile belongs to ONE policy (EvalArgs: policy = tile / tiles_per_policy, wave-uniform, formed once in the prologue): it
// loads that policy's weights and flies the block's first envs_per_policy envs; the padding envs behind them are never live.  The wave keeps feeding them through the actor — the MFMAs need the whole wave — and discards what comes out; it leaves
// the loop as soon as no lane is live (a ballot: the loop condition stays wave-uniform), so a crashing policy costs only as many
// steps as its longest-surviving env.  Frozen lanes fly on unaccounted; nothing they compute reaches memory or another lane (each
// env is one column of the actor's GEMMs).  Every evaluated step starts in regime (the lane stops at the first observation with
// |eW| >= 1), so the rate-adaptive path cannot trigger and the plain integrator is the step_kernel arithmetic of these envs.
template <int KIND, typename XV, typename QW, int TRAJ, bool MAG>
__global__ __launch_bounds__(64, 1) void eval_kernel(const EvalLaunch in) {
#if defined(__HIP_DEVICE_COMPILE__)
  // (as in step_kernel: fields are read from the kernarg segment where they are used, not held in SGPRs across the loop)
  const EvalLaunch& kin = *reinterpret_cast<const EvalLaunch*>(__builtin_amdgcn_kernarg_segment_ptr());
  (void)in;
#else
  const EvalLaunch& kin = in;  // (host pass of the single-source compile: never executed)
#endif
  const Args& ka = kin.a;
  const EvalArgs& ke = kin.e;
  using T = QW;
  using X = XV;
  using KT = KindTraits<KIND>;
  static_assert(KIND != QR_KIND_QUAD, "the wrappers only: Quad-v0 has no actor");
  constexpr int A = KT::A, D0 = KT::D0, D1 = KT::D1 ? KT::D1 : 1, NAG = KT::NAG;
  constexpr bool kStateful = TRAJ == 2;
  __shared__ __attribute__((aligned(16))) float smem[64 * D0];
  using Actor1 = ActorLds<3, 4, 1>;
  __shared__ __attribute__((aligned(16))) float wsm[KT::D1 > 0 ? Actor1::SIZE : 4];
  const int tid = threadIdx.x;
  const unsigned lane = threadIdx.x;
  const unsigned ufirst = blockIdx.x * 64u;
  const int64_t first = (int64_t)ufirst;
  const int64_t i = first + tid;
  const int64_t L = ka.ld;
  const unsigned tpp = (unsigned)ke.tiles_per_policy;
  const unsigned policy = blockIdx.x / tpp;  // wave-uniform
  const int rows = min(ke.envs_per_policy - (int)((blockIdx.x - policy * tpp) * 64u), 64);
  const bool active = tid < rows;
  const unsigned ll = min(lane, (unsigned)(rows - 1));  // lanes past a ragged tail read the tail's last env and are never live
  const Coeffs& c = ka.c;

  // ---- the env's working set ----
  Work<T, X> w;
  load_state<XV, QW>(ka, first, ll, w);
  w.nominal = ka.params == nullptr;
  {
    const SoA<float> prm(ka.params, 6, L);
#pragma unroll
    for (int f = 0; f < 6; ++f) w.prm[f] = prm.load(f, ufirst, ll);
    const SoA<float> integ(ka.integ, 8, L);
#pragma unroll
    for (int f = 0; f < 8; ++f) w.integ[f] = integ.load(f, ufirst, ll);
  }
  hover_goal(w.goal);
  if ((!TRAJ || kStateful) && ka.goal != nullptr) {  // (stateless generator modes form the goal in registers every step)
    const SoA<float> goal(ka.goal, 12, L);
#pragma unroll
    for (int f = 0; f < 12; ++f) w.goal[f] = goal.load(f, ufirst, ll);
  }
  Traj tr;
  const int goal_mode = TRAJ ? ka.goal_mode : QR_GOAL_EXTERNAL;
  if constexpr (TRAJ) {
    const SoA<float> traj(ka.traj, 8, L);
#pragma unroll
    for (int f = 0; f < (kStateful ? 8 : 7); ++f) tr.set(f, traj.load(f, ufirst, ll));
  }

  // ---- the actor(s) and the first observation ----
  float po0[D0], po1[D1];
  ActorMfma<D0, true> actor0;  // (the host clears the log_std sources: only the mean head is formed)
  load_rows<64, D0>(ka.obs0_in + first * D0, po0, smem, tid, rows);
  if constexpr (KT::D1 > 0) load_rows<64, D1>(ka.obs1_in + first * D1, po1, smem, tid, rows);
  actor0.load(actor_of_policy<D0, 16, 4>(ka.actor[0], policy), tid);
  if constexpr (KT::D1 > 0) Actor1::fill(wsm, actor_of_policy<3, 4, 1>(ka.actor[1], policy), tid);
  tile_sync<64>();

  bool live = active;
  double ret[NAG], bsum = 0.0;
#pragma unroll
  for (int g = 0; g < NAG; ++g) ret[g] = 0.0;
  const int max_steps = ke.max_steps;
  for (int t = 0; t < max_steps; ++t) {
    // ---- deterministic action (qr_rollout_actor with deterministic != 0: ppo.py:100-101, td3.py:93-96 at std 0, sac.py:104-105) ----
    float pre[A], ls[A], eps[A], act[A], logp[A];
#pragma unroll
    for (int j = 0; j < D0; ++j) smem[tid * D0 + j] = po0[j];
    tile_sync<64>();
    {
      float p0[4], l0[4];
      actor0.heads(smem, tid, p0, l0);
#pragma unroll
      for (int j = 0; j < 4; ++j) { pre[j] = p0[j]; ls[j] = l0[j]; }
    }
    if constexpr (KIND == QR_KIND_DECOUPLED) {
      float p1[1], l1[1];
      Actor1::heads(wsm, false, po1, p1, l1);
      pre[A - 1] = p1[0]; ls[A - 1] = l1[0];
    }
    tile_sync<64>();  // the tile is written again at the next step
#pragma unroll
    for (int j = 0; j < A; ++j) eps[j] = 0.0f;
    actor_sample<4, true>(ka.actor[0].squash, false, &pre[0], &ls[0], &eps[0], true, ka.max_action, &act[0], &logp[0]);
    if constexpr (A > 4) actor_sample<1, true>(ka.actor[1].squash, false, &pre[A - 1], &ls[A - 1], &eps[A - 1], true, ka.max_action, &act[A - 1], &logp[A - 1]);

    // ---- goal from the pre-step state, action map, integration over dt ----
    if constexpr (TRAJ) {
      float b1d_dot[3];
      traj_goal<kStateful>(w, tr, goal_mode, c, b1d_dot);
    }
    ActConsts<T> ac;
    act_consts(w, c, ac);
    Dyn<T> dyn;
    action_map<KIND, T, X>(act, w, ac, c, dyn);
    const int nsub = ka.substeps;
    integrate_sel<MAG>(w.x, w.v, w.q, w.W, dyn, nsub, T(c.dt) * recip(T(nsub)));
    renorm_quat(w.q);

    // ---- observation, reward, done (as step_kernel's wrapper branch) ----
    T R[9];
    float o0[D0], o1[D1];
    float rraw[NAG], rwd[NAG];
    bool dn[NAG];
    quat_to_R(w.q, R);
    error_obs<KIND, T, X>(w, R, c, o0, o1);
    wrapper_reward_done<KIND>(o0, o1, c, rraw, rwd, dn);
    bool any_done = false;
#pragma unroll
    for (int g = 0; g < NAG; ++g) {
      if (dn[g]) rwd[g] = -1.0f;  // crash override (quad.py:162-166)
      any_done = any_done | dn[g];
    }
    QuatPack<T> qp;
    pack_quat(w.q, qp);
    unpack_quat(qp, w.q);  // the next env-step starts from what a single-step launch would have re-loaded

    // ---- eval_policy's accounting (main.py:353-373), in float64 ----
    // get_error_state (utils/utils.py:21-38): ex = obs[0:3] x_lim, eb1 = obs[18] (MONO) / obs2[0] (MODUL) pi, from the float32 rows
    double ex[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) ex[j] = (double)o0[j] * c.x_lim;
    const double eb1 = (double)(KIND == QR_KIND_COUPLED ? o0[18] : o1[0]) * kPi;
    // benchmark_reward_func: interp(-|ex| - |eb1|, [-2, 0], [0, 1]) — the sum is never positive, so only the lower end clamps
    const double brw = -sqrt(ex[0] * ex[0] + ex[1] * ex[1] + ex[2] * ex[2]) + -fabs(eb1);
    const double bstep = brw < -2.0 ? 0.0 : 0.5 * (brw + 2.0);
    if (live) {
#pragma unroll
      for (int g = 0; g < NAG; ++g) ret[g] += (double)rwd[g];
      bsum += bstep;
    }
    const bool full = t + 1 == max_steps;
    if (live && (any_done || full)) {  // ---- this lane's episode ends here: write it back, once ----
      store_state<XV, QW>(ka, first, lane, w, qp);
      const SoA<float> integ(ka.integ, 8, L);
#pragma unroll
      for (int f = 0; f < 8; ++f) integ.store(f, ufirst, lane, w.integ[f]);
      if constexpr (TRAJ) {
        const SoA<float> traj(ka.traj, 8, L);
        traj.store(0, ufirst, lane, tr.calls);
        if constexpr (kStateful) {  // (the stateless modes change nothing but the call counter between episode starts)
#pragma unroll
          for (int f = 1; f < 8; ++f) traj.store(f, ufirst, lane, tr.get(f));
          const SoA<float> goal(ka.goal, 12, L);
#pragma unroll
          for (int f = 0; f < 12; ++f) goal.store(f, ufirst, lane, w.goal[f]);
        }
      }
      if (int32_t* const steps_ptr = ka.steps) steps_ptr[i] += t + 1;
#pragma unroll
      for (int j = 0; j < D0; ++j) ka.obs0[i * D0 + j] = o0[j];
      if constexpr (KT::D1 > 0) {
#pragma unroll
        for (int j = 0; j < D1; ++j) ka.obs1[i * D1 + j] = o1[j];
      }
      if (float* const ao = ka.act_out) {
#pragma unroll
        for (int j = 0; j < A; ++j) ao[i * A + j] = act[j];
      }
      const bool sx = full && fabs(ex[0]) <= 0.01 && fabs(ex[1]) <= 0.01 && fabs(ex[2]) <= 0.01;
#pragma unroll
      for (int g = 0; g < NAG; ++g) {
        ke.ret[i * NAG + g] = ret[g];
        ke.success[i * NAG + g] = (uint8_t)((g == 0 ? sx : (full && fabs(eb1) <= 0.01)) ? 1 : 0);
      }
      ke.bench[i] = bsum;
      ke.length[i] = t + 1;
      ke.terminated[i] = (uint8_t)(any_done ? 1 : 0);
      if (float* const fe = ke.final_error) {
#pragma unroll
        for (int j = 0; j < 3; ++j) fe[i * 4 + j] = (float)ex[j];
        fe[i * 4 + 3] = (float)eb1;
      }
      live = false;
    }
    if (__ballot(live) == 0) break;  // wave-uniform: every lane of the tile is frozen
#pragma unroll
    for (int j = 0; j < D0; ++j) po0[j] = o0[j];
#pragma unroll
    for (int j = 0; j < D1; ++j) po1[j] = o1[j];
  }
}

}  // namespace qr
