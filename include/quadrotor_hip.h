/*
 * quadrotor_hip.h — C-ABI of the MI355X-native batched quadrotor dynamics engine.
 *
 * Drop-in boundary for ONE hot path of fdcl-gwu/gym-rotor: env.step() of Quad-v0 /
 * CoupledWrapper / DecoupledWrapper (the template method QuadEnv.step,
 * gym_rotor/envs/quad.py:142-168, and the hooks it calls), batched over N independent
 * quadrotors that live in device memory.  The reference is pure Python and has no
 * native layer, so each entry point below names the reference *method* it replaces.
 *
 * Conventions
 *   - plain C: pointers, sizes, PODs; no torch / C++ types.  All pointers are DEVICE
 *     pointers (HBM) unless stated otherwise.  `stream` is a hipStream_t passed as void*
 *     (NULL = the default stream).  Every call is asynchronous on `stream`.
 *   - return value: 0 on success; <0 = argument error (QR_E_*); >0 = hipError_t of the
 *     launch.  Nothing is ever computed on the host: there is no CPU fallback.
 *   - layout: per-env quantities are SoA, `field-major [F][N]` (lane i touches
 *     base[f*N + i], so a 64-lane wavefront reads 256/512 contiguous bytes per field).
 *     With field_stride = L the address is base[f*L + i].
 *     Caller-facing rows (actions in, observations/reward/done out) are AoS `[N][D]`
 *     row-major, i.e. what a policy network produces/consumes; the kernels transpose
 *     through LDS so that those rows are written with coalesced 16-byte stores.
 *   - INTERNAL STATE (12 words per env instead of the reference's 18): the step is
 *     HBM/fabric-bound, so the rotation is kept as a unit quaternion, which the kernel
 *     integrates directly (q' = q (0,W)/2 is the same flow as R' = R hat(W),
 *     quad.py:328) and stores as its THREE components of smaller magnitude ("smallest
 *     three": the dropped one is made positive and rebuilt as sqrt(1 - sum of squares) >= 1/2;
 *     its index rides in the two lowest mantissa bits of the first stored component):
 *         pos_vel  [6][N]  x(3), v(3)
 *         att_rate [6][N]  k0, k1, k2 of q = (w,x,y,z) with R = R(q); W(3)
 *     An all-zero att_rate is the identity attitude at rest.
 *     The reference's 18-vector (x, v, vec_F(R) column-major, W; quad.py:146,
 *     quad_utils.py:12-16) is produced / consumed by qr_get_state / qr_set_state.
 *   - precision (`layout`): QR_LAYOUT_MIXED (default) stores x,v as float32 and q,W as
 *     float64; W is integrated and q ACCUMULATED in float64, the RK4 stage quaternions and
 *     the thrust direction are formed in float32 (same 1000-step error as
 *     all-float64 arithmetic).  QR_LAYOUT_F64 stores and computes everything in float64 (the
 *     reference-grade mode: 4th-order convergence to the reference down to 1e-10);
 *     QR_LAYOUT_F32 stores and computes in float32 (fast, NOT inside the 1e-5/1000-step
 *     parity bar).  See DESIGN.md §4 for the measurements behind this.
 */
#ifndef QUADROTOR_HIP_H
#define QUADROTOR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QR_ABI_VERSION 16

/* env kinds */
#define QR_KIND_QUAD      0 /* QuadEnv            gym_rotor/envs/quad.py:19            */
#define QR_KIND_COUPLED   1 /* CoupledWrapper     wrappers/coupled_yaw_wrapper.py:11   */
#define QR_KIND_DECOUPLED 2 /* DecoupledWrapper   wrappers/decoupled_yaw_wrapper.py:12 */

/* state layouts */
#define QR_LAYOUT_MIXED 0 /* pos_vel float32, att_rate float64; float64 W + q accumulation, float32 RK4 stages */
#define QR_LAYOUT_F64   1 /* all float64                                           */
#define QR_LAYOUT_F32   2 /* all float32                                           */

/* argument errors */
#define QR_E_NULL   (-1) /* a required pointer is NULL             */
#define QR_E_KIND   (-2) /* kind / layout / actor.squash out of range, or an entry point undefined for the kind */
#define QR_E_SIZE   (-3) /* num_envs < 0 or > 22 369 621 (32-bit SoA offsets), bad field_stride, substeps < 1, n_steps < 1,
                            or a QrCoeffs with non-positive nominal parameters / dt (not filled by qr_default_coeffs) */
#define QR_E_ALIGN  (-4) /* a buffer is not 16-byte aligned        */

/* goal sources */
#define QR_GOAL_EXTERNAL 0 /* goal buffer set by the caller (set_goal_state), or the hover default    */
#define QR_GOAL_MODE0    1 /* TrajectoryGenerator mode 0: xd = vd = 0, b1d drawn at episode start     */
#define QR_GOAL_MODE1    2 /* TrajectoryGenerator mode 1: exponential approach of the origin + yaw rate */
#define QR_GOAL_MODE6    3 /* TrajectoryGenerator mode 6: eight-shaped (Lissajous) curve (:418-505); after
                              eight_count periods the last goal is held (the reference switches to manual) */
/* The STATEFUL modes (:279-416): the generator object carries xd, vd, b1d, b1d_dot, Wd and its flags from call to call (a mode
 * writes only the components it moves; after completion it switches to manual mode, which holds position and heading and no
 * longer recomputes Wd).  They need QrEnv.goal: xd, vd, b1d, Wd persist THERE; b1d_dot, the flags and x_init in QrEnv.traj. */
#define QR_GOAL_MODE2    4 /* mode 2 take-off: climb at 0.05 m/s from the start position to the height -0.5 m, then manual    */
#define QR_GOAL_MODE3    5 /* mode 3 landing: descend at 1 m/s to the motor cut-off height -0.25 m                            */
#define QR_GOAL_MODE4    6 /* mode 4 stay: hold the current position and heading (manual mode from the second call on)        */
#define QR_GOAL_MODE5    7 /* mode 5 circle: 1.75 s run-up along +x, two circles of radius 0.7 m at 0.4 rad/s, then manual    */
/* Two deviations of the stateful modes (2-5) from the reference's long-lived TrajectoryGenerator object, both bounded:
 *  (1) Episode start.  mark_traj_start (trajectory_generator.py:176-191) keeps xd, vd, b1d, b1d_dot, Wd of the PREVIOUS episode on
 *      the object; here every episode starts from a fresh generator (xd = vd = Wd = 0, b1d = e1, b1d_dot = 0).  Modes 2-4
 *      overwrite all of them in their first call, so only mode 5 can tell: an episode that ended mid-circle would carry
 *      b1d_dot != 0 into the next run-up, i.e. a non-zero Wd for the first call (|Wd_3| <= 0.4 rad/s), until the run-up branch
 *      rewrites b1d_dot at that same call's end.  (A per-env generator has no "previous object"; the oracle models the same.)
 *  (2) Phase boundaries.  The generator's clock is t = calls * dt formed in float32; the reference accumulates t += dt in
 *      float64 (:224-229).  A phase test `t < t_switch` therefore flips at the same call unless t_switch lies within ~1e-6 s
 *      of a multiple of dt — then one call early or late: a one-step goal error of at most |v| dt (take-off 0.25 mm, landing
 *      5 mm, circle run-up 2 mm).  The one boundary that IS an exact multiple of the default dt (the circle's run-up, 350 dt)
 *      is matched to the reference's accumulated value (1.7499999999999847 s: still run-up).  Pinned by the closed-loop
 *      goldens for the default dt (tests/test_closedloop_td3.py); other dt: the bound above. */

/* flags */
#define QR_FLAG_AUTO_RESET   1u /* re-sample a done env inside the same launch (train distribution) */
#define QR_FLAG_EVAL_RESET   2u /* resets use env_type='eval' (quad.py:352-356) instead of 'train' */
#define QR_FLAG_NO_UDM       4u /* resets keep nominal parameters (use_UDM False / eval)            */
#define QR_FLAG_CALLER_RESETS 32u /* WITHOUT QR_FLAG_AUTO_RESET: the caller promises the reference's own loop (main.py:183-186,
                                    212-230): every env a step reports done is reset (qr_reset / qr_set_state) before it is stepped
                                    again.  Then no env ever starts a step outside the termination bounds, rate adaptivity
                                    (QrCoeffs.w_adapt) cannot trigger, and the launcher takes the kernel compiled without it — the
                                    same arithmetic, bit for bit, as with QR_FLAG_AUTO_RESET (4.03 instead of 4.39 us per 65 536-env
                                    launch).  A caller that steps done envs on anyway only loses the adaptivity: fixed substeps.
                                    Honoured by ONE-STEP launches only (qr_step): inside a qr_rollout / qr_rollout_actor launch of
                                    several steps nobody can reset an env between two of them, so those keep the rate-adaptive kernel. */
/* Launch-rule overrides (speed only: no choice changes a result bit).  By default qr_step / qr_rollout(_actor) decide from the
 * grid size whether every 64-env tile gets a second, helper wavefront, with thresholds measured on MI355X (environment variables
 * QR_HELPER_GRID, QR_HELPER_GRID_WRAP, QR_HELPER_GRID_ROLLOUT override them per process, read once); these bits pin the choice
 * per env — what an autotuner that timed both on ITS box, kind, size and action source sets.  Ignored where the instantiation
 * does not exist (a helper wavefront needs QR_FLAG_AUTO_RESET, the default layout and no rate adaptivity in reach). */
#define QR_FLAG_FORCE_HELPER   8u /* qr_step: a helper wavefront per 64-env tile whatever the grid size */
#define QR_FLAG_NO_HELPER     16u /* qr_step: never                                                     */
#define QR_FLAG_FORCE_HELPER_ROLLOUT  64u /* the same two for the multi-step launches (qr_rollout, qr_rollout_actor), whose crossover  */
#define QR_FLAG_NO_HELPER_ROLLOUT    128u /* is a different one (two waves per SIMD): a choice timed on one family says nothing about the other */
/* (qr_rollout_actor on grids beyond that crossover runs the helper-wave instantiation over chunks of resident tiles, one launch after
 *  the other, unless QR_FLAG_NO_HELPER_ROLLOUT is set: the same results, 18-22 % less time at 98 304 ... 262 144 envs.) */

/* Coefficients a caller may override (args_parse.py:23-35); qr_default_coeffs() fills the
 * reference defaults.  reward_min* are derived inside (quad.py:81-88). */
typedef struct QrCoeffs {
  double Cx, CIx, Cv, Cb1, CIb1, CW;  /* MONO / Quad-v0 reward (CW = Cw12, quad.py:80) */
  double Cw12, CW3;                   /* MODUL                                         */
  double alpha, beta;                 /* integral leak terms (quad.py:448-450)         */
  double dt;                          /* 1/200 s (quad.py:60-61)                       */
  double x_lim, v_lim, W_lim;         /* 1.0, 4.0, 2*pi (quad.py:104-106)              */
  double eIx_lim, eIb1_lim;           /* 3.0, 3.0 (coupled_yaw_wrapper.py:23-24)       */
  double euler_lim_deg;               /* 85 (quad.py:107)                              */
  double udm_fraction;                /* UDM_percentage/100 = 0.1 (quad.py:370)        */
  /* eight-shaped curve of the goal generator (utils/trajectory_generator.py:98-110) */
  double eight_T, eight_A1, eight_A2; /* period 9 s, amplitudes 1.5 / 1.0                  */
  double eight_w_b1d, eight_alt_d;    /* yaw rate 0.349066 rad/s, desired altitude -0.6 m  */
  double eight_eps, eight_count;      /* smoothing epsilon 0.01, number of eights 3        */
  /* Rate-adaptive substepping (the fixed-step stand-in for DOP853's error control, quad.py:265):
   * a wavefront (64 consecutive envs) containing an env whose body rate max|W_i| exceeds w_adapt
   * takes ceil(max|W_i| / w_adapt) times the requested substeps (capped at 16x), so envs that
   * are stepped on far beyond termination (free run, no AUTO_RESET) keep the 1e-5 trajectory
   * bar.  Default 16 rad/s ~ 2.5x the termination bound W_lim = 2 pi: in-regime envs always take
   * exactly `substeps`, and with QR_FLAG_AUTO_RESET (every env is re-sampled when its rate
   * error leaves its bound; goal rates |Wd| <= W_lim / 2) it can never trigger, so the launcher
   * then uses the kernel compiled without it.  0 disables it. */
  double w_adapt;
  /* Nominal vehicle and environment constants (QuadEnv.__init__, quad.py:28-36): what a reset without
   * domain randomisation restores, what UDM scatters around, and what an env without a params
   * buffer flies with. */
  double m_nominal, d_nominal, J1_nominal, J3_nominal; /* 2.15 kg, 0.23 m, 0.022 (= J2), 0.035 kg m^2 */
  double c_tf_nominal, c_tw_nominal;                   /* 0.0135, 2.2                                 */
  double g, min_force;                                 /* 9.81 m/s^2, 0.5 N                           */
} QrCoeffs;

/* Per-env device buffers owned by the caller (the Python env object). */
typedef struct QrEnv {
  int32_t kind;        /* QR_KIND_*                                                       */
  int32_t layout;      /* QR_LAYOUT_*                                                     */
  int64_t num_envs;    /* N                                                               */
  int64_t field_stride;/* elements between consecutive fields of EVERY SoA buffer below; 0 = N.
                          A multiple of 4, >= N.  Padding it off a power of two avoids all
                          fields of an env landing on one HBM channel.        */
  int64_t env_offset;  /* global id of local env 0 (multi-GPU shard offset; RNG key)      */
  uint64_t seed;       /* RNG seed.  qr_reset draws depend only on (seed, global env id, episode); in-launch
                          resets (QR_FLAG_AUTO_RESET) on (seed, global id of the 64-env tile's first env,
                          reset_count of that tile, rank of the env among the tile's envs that reset in
                          that step) — see reset_count                                                */
  void*    pos_vel;    /* [6][N]  x, v                                         in/out      */
  void*    att_rate;   /* [6][N]  q (smallest three), W                        in/out      */
  float*   integ;      /* [8][N]  eIx(3), g_x prev(3), eIb1, g_b prev (quad_utils.py:38-63); NULL for QUAD */
  float*   params;     /* [6][N]  m,d,J1(=J2),J3,c_tf,c_tw (quad.py:359-387); NULL = nominal */
  float*   goal;       /* [12][N] xd,vd,b1d,Wd (quad.py:413-418); NULL = hover default     */
  float*   traj;       /* [8][N]  goal-generator state, required when goal_mode != QR_GOAL_EXTERNAL:
                          0 #get_desired calls since mark_traj_start (t = calls*dt), 1 theta_init,
                          2,3 b1d x,y (mode 0) | w_b1d, smooth_term (mode 1) | b1d_dot x, flags (modes 2-5),
                          4..6 x_init, 7 b1d_dot y (modes 2-5) */
  int32_t  goal_mode;  /* QR_GOAL_EXTERNAL (0), or a utils/trajectory_generator.py mode fused into
                          the step: QR_GOAL_MODE0 idle/warm-up (:141-148), QR_GOAL_MODE1 hovering (:252-277),
                          QR_GOAL_MODE6 eight-shaped curve (:418-505), QR_GOAL_MODE2..5 take-off / landing / stay /
                          circle (:279-416; these need `goal`) */
  int32_t  reserved0;
  int32_t* episode;    /* [N]     episode counter (RNG stream id); required for resets     */
  int32_t* steps;      /* [N]     steps since reset; NULL = no time-limit bookkeeping      */
  int32_t* reset_count;/* [ceil(N/64)] stream position of the in-launch reset of each 64-env tile (one
                          wavefront): advanced by 1 per env-step by qr_step / qr_rollout(_actor) with
                          QR_FLAG_AUTO_RESET (required then), so that a (tile, count) pair is never
                          used twice — also when a captured hipGraph is replayed.  The draws of tile
                          j depend only on (seed, env_offset + 64 j, count, slot): results do not
                          depend on how the batch is sharded as long as every shard starts at a
                          multiple of 64 envs.  Zero-initialise.                                     */
  int32_t  max_episode_steps; /* >0: truncated[i]=1 when steps reaches it (gym_rotor/__init__.py:3-7) */
  uint32_t flags;      /* QR_FLAG_*                                                       */
  QrCoeffs coeffs;
} QrEnv;

/* Outputs of one step, all AoS rows.  obs0 is float32 [N][18] (QUAD: the next state in the
 * reference's order, quad.py:269-271; optional), [N][23] (COUPLED) or [N][15] (DECOUPLED
 * agent 1); obs1 is [N][3] (DECOUPLED agent 2) else NULL.  reward/done are [N][n_agents],
 * n_agents = 2 for DECOUPLED, else 1. */
typedef struct QrStepOut {
  float*   obs0;        /* QUAD: may be NULL (no observation rows written)                */
  float*   obs1;
  float*   reward;      /* normalised to [0,1], -1 on crash (quad.py:154-166)             */
  float*   reward_raw;  /* optional: hook output before np.interp / crash override        */
  uint8_t* done;        /* terminated flags (done_wrapper)                                */
  uint8_t* truncated;   /* optional [N]                                                   */
  /* Optional, with QR_FLAG_AUTO_RESET: rows [N][D0] / [N][D1] (same shapes as obs0 / obs1; QUAD: [N][18])
   * that receive the TERMINAL observation of every env that is re-sampled in this step — the
   * obs_next the reference stores for that transition (main.py:163-175; obs0/obs1 then already hold
   * the first observation of the new episode).  Rows of envs that did not reset are left untouched. */
  float*   final_obs0;
  float*   final_obs1;
} QrStepOut;

/* Replaces QuadEnv.step(action) (quad.py:142-168) = action_wrapper -> observation_wrapper
 * (ODE solve over dt + get_norm_error_state) -> reward_wrapper -> interp -> done_wrapper ->
 * crash override, for all N envs in one fused launch.
 *   action   [N][A] float32, A = 4 (QUAD, COUPLED) or 5 (DECOUPLED: agents' actions
 *            concatenated, main.py:161).  16-byte aligned (A = 4) / 4-byte aligned (A = 5).
 *   substeps number of fixed 4th-order substeps of h = dt/substeps replacing
 *            scipy.integrate.solve_ivp(DOP853) (quad.py:265); >= 1.  ONE substep is an RK4 step; with two or more the default
 *            layout takes a Lie-group (Magnus) substep of the same order at half the instructions (qr_dynamics.h; the uniform
 *            layouts stay RK4).  The choice rides on `substeps` alone, never on the batch size or the launch family: a shard, a
 *            rollout and an actor rollout compute the bits of the global, per-step launches of the same `substeps`. */
int qr_step(const QrEnv* env, const float* action, int32_t substeps, const QrStepOut* out, void* stream);

/* K env-steps in ONE launch with the state held in registers between steps:
 *   action [K][N][A]; outputs [K][N][...] (pointers in `out` are the t=0 slices, the
 *   per-step strides are the full [N][..] extents).  Same maths as K calls of qr_step. */
int qr_rollout(const QrEnv* env, const float* action, int32_t n_steps, int32_t substeps,
               const QrStepOut* out, void* stream);

/* One MLP actor of the reference: fc1 -> relu -> fc2 -> relu -> heads.  Device pointers to float32
 * tensors in torch.nn.Linear layout (weight [out][in] row-major), i.e. `actor.fc1.weight.data_ptr()`
 * etc. as they are.
 *   QR_ACTOR_TANH_MEAN   PPO  MLP_Actor_PPO (algos/ppo/ppo_mlp.py:6-58) and TD3 MLP_Actor_TD3
 *                        (algos/td3/td3_mlp.py:5-34, mean head = fc3): mean = tanh(head(h));
 *                        action = clamp(mean + exp(log_std) eps, +-max_action)  (ppo.py:93-99, td3.py:93-96)
 *   QR_ACTOR_TANH_SAMPLE SAC  MLP_Actor_SAC (algos/sac/sac_mlp.py:16-82): mean = mean_linear(h),
 *                        log_std = clamp(log_std_linear(h), -20, 2); action = tanh(mean + exp(log_std) eps)
 * log_std: the state-independent parameter [action_dim] (PPO; TD3: log of the exploration std) —
 * or, when log_std_w is set, the second head log_std_w [action_dim][hidden], log_std_b [action_dim]. */
#define QR_ACTOR_TANH_MEAN   0
#define QR_ACTOR_TANH_SAMPLE 1
typedef struct QrActor {
  const float* fc1_w;   const float* fc1_b;   /* [hidden][obs_dim], [hidden]        */
  const float* fc2_w;   const float* fc2_b;   /* [hidden][hidden],  [hidden]        */
  const float* mean_w;  const float* mean_b;  /* [action_dim][hidden], [action_dim] */
  const float* log_std;                        /* [action_dim], or NULL with a log_std head */
  const float* log_std_w; const float* log_std_b; /* optional state-dependent log_std head  */
  int32_t obs_dim, hidden_dim, action_dim;
  int32_t squash;                              /* QR_ACTOR_TANH_MEAN | QR_ACTOR_TANH_SAMPLE */
} QrActor;

/* Caller side of a PPO collection loop (main.py:141-166 with PPO.choose_action, ppo.py:82-101)
 * for qr_rollout_actor. */
typedef struct QrPolicyRollout {
  const QrActor* actors;  /* host array, one per agent with the reference's default sizes
                             (args_parse.py:40): COUPLED 1 actor 23->16->16->4; DECOUPLED 2 actors
                             15->16->16->4 and 3->4->4->1.  Other sizes: QR_E_SIZE.             */
  const float* obs0_in;   /* [N][D0] observation the FIRST action is computed from (what the
                             last step / reset + get_norm_error_state returned)                */
  const float* obs1_in;   /* [N][3], DECOUPLED only                                            */
  const float* noise;     /* optional [K][N][A] standard-normal draws eps (action = mean + std
                             eps: reproduces a given torch sample; tests).  NULL = drawn in the
                             kernel: Philox4x32-10 keyed by (noise_seed, global env id,
                             step_base + t) + Box-Muller, independent of the sharding.         */
  uint64_t noise_seed;
  uint64_t step_base;     /* global step index of t = 0 (advance by K per call)               */
  float max_action;       /* clamp (args_parse.py:45: 1.0)                                    */
  int32_t deterministic;  /* != 0: action = clamp(mean) resp. tanh(mean) (is_eval: ppo.py:100-101, sac.py:104-105) */
  float* action_out;      /* [K][N][A] actions taken (agents concatenated, main.py:161)       */
  float* logprob_out;     /* [K][N][A] per component: TANH_MEAN Normal(mean, std).log_prob(action) of the
                             CLAMPED action (ppo.py:97-98); TANH_SAMPLE Normal.log_prob(u) - log(1 -
                             action^2 + 1e-6), u the pre-tanh sample (sac_mlp.py:74-77).  NULL allowed */
} QrPolicyRollout;

/* K env-steps in ONE launch with the policy inside the loop: per step, each env's actor(s) are
 * evaluated on its current observation (registers), the action is sampled, clamped and stepped,
 * and obs / action / logprob / reward / done rows are written as [K][N][..] (what
 * algos/replay_buffer.py:20-39 stores per step).  `out` as in qr_rollout (obs rows required):
 * out->obs0[t] is the observation AFTER step t, i.e. the input of step t+1.  COUPLED and
 * DECOUPLED only (the reference trains on the wrappers). */
int qr_rollout_actor(const QrEnv* env, const QrPolicyRollout* policy, int32_t n_steps, int32_t substeps,
                     const QrStepOut* out, void* stream);

/* Per-env results of qr_evaluate_actor (NAG = 2 for DECOUPLED, else 1). */
typedef struct QrEvalOut {
  double*  episode_return; /* [N][NAG] sum of rewards up to and including the terminal step (main.py:356; summed in float64, where
                              the reference rounds the running sum to 4 decimals every step) */
  double*  benchmark;      /* [N]      sum of benchmark_reward_func(ex, eb1) (utils/utils.py:42-47) */
  int32_t* length;         /* [N]      steps taken (1..max_steps) */
  uint8_t* terminated;     /* [N]      1 = ended by done (any agent), 0 = ran max_steps without */
  uint8_t* success;        /* [N][NAG] length == max_steps and |ex|_inf <= 0.01 (agent 0), |eb1| <= 0.01 (MODUL agent 1), judged at the
                              last step (main.py:366-373).  Deliberate deviation: the reference never clears its `success` list between
                              episodes, so an episode that ends early re-appends the flags of the episode before it; here such an
                              episode has success = 0. */
  float*   final_error;    /* [N][4]   ex (3), eb1 of the last step, as get_error_state forms them; may be NULL */
  float*   obs0; float* obs1; /* final observation rows [N][D0] / [N][D1] (DECOUPLED: obs1 required) */
} QrEvalOut;

/* Replaces Learner.eval_policy (main.py:270-404) for N envs in ONE launch: from each env's CURRENT state, its observation
 * policy->obs0_in / obs1_in and its goal (buffer or fused generator), up to max_steps env-steps of the deterministic action
 * (QrPolicyRollout.deterministic != 0's rule; noise, deterministic and logprob_out are ignored) until the first step that sets
 * any agent's done flag — that step included.  Then the env freezes: its state, integrators, generator state and goal stop
 * changing and are written back, `steps` (when present) advances by `length`, and its final observation rows, last action
 * (policy->action_out, optional: [N][A]) and results go to `out`.  No per-step row is written, nothing is re-sampled
 * (QR_FLAG_AUTO_RESET and max_episode_steps are ignored), and a 64-env tile stops as soon as all of its envs are frozen.
 * Every evaluated step starts in regime, so the plain integrator runs (RK4; Magnus for substeps >= 2 in the default layout,
 * the same rule as every other launch).  COUPLED and DECOUPLED only (QR_E_KIND for Quad-v0); QR_E_SIZE for max_steps < 1 or
 * actor sizes other than qr_rollout_actor's. */
int qr_evaluate_actor(const QrEnv* env, const QrPolicyRollout* policy, int32_t max_steps, int32_t substeps,
                      const QrEvalOut* out, void* stream);

/* The block layout of qr_evaluate_population: P policies, E episodes each, on ONE env of N = P * Epad envs, Epad = E rounded up
 * to a multiple of 64 (a 64-env tile never holds two policies).  Policy p owns envs [p * Epad, p * Epad + E); the Epad - E
 * padding envs behind them are never flown. */
typedef struct QrPopulation {
  int32_t n_policies;       /* P >= 1 */
  int32_t envs_per_policy;  /* E >= 1; env->num_envs must equal P * roundup(E, 64) */
} QrPopulation;

/* qr_evaluate_actor for P policies in ONE launch (checkpoint selection, sweeps, the fitness of a perturbed population): the same
 * kernels, arithmetic, freeze and write-back per env; only the weights differ per block.  Stacked-tensor rule: every tensor of
 * policy->actors[k] is a contiguous float32 [P][...] stack of the per-policy tensors of QrActor's sizes; the QrActor pointers
 * point at policy 0 and policy p's tensor starts p * numel elements later (fc1_w [P][hidden][obs_dim], fc1_b [P][hidden], ...).
 * The log_std sources are never read (one of them must still be set, as for qr_evaluate_actor) and squash is shared.
 * policy->obs0_in / obs1_in, policy->action_out and every array of `out` are indexed by env, [N][...], as in qr_evaluate_actor;
 * padding rows are ignored on input and untouched on output, and so are the padding envs' state, integrators, generator state
 * and `steps`.  n_policies = 1 with envs_per_policy = N is qr_evaluate_actor, bit for bit.  QR_E_NULL for a NULL pop; QR_E_SIZE
 * for P < 1, E < 1 or num_envs != P * roundup(E, 64); every other check is qr_evaluate_actor's. */
int qr_evaluate_population(const QrEnv* env, const QrPolicyRollout* policy, const QrPopulation* pop, int32_t max_steps,
                           int32_t substeps, const QrEvalOut* out, void* stream);

/* Replaces QuadEnv.get_norm_error_state(framework) (quad.py:421-466): normalised error
 * observation of the CURRENT state; advances both trapezoid integrators (same side
 * effect as the reference).  kind must be COUPLED or DECOUPLED. */
int qr_error_obs(const QrEnv* env, float* obs0, float* obs1, void* stream);

/* The same with the FORMAT chosen by the caller, as the reference's `framework` argument does (quad.py:452-466: "MONO" ->
 * one [N][23] row, "MODUL" -> [N][15] + [N][3], on whichever wrapper class the method is called): format = QR_KIND_COUPLED
 * (MONO; obs1 unused) or QR_KIND_DECOUPLED (MODUL; obs1 required), independent of env->kind.  env->kind must still be COUPLED
 * or DECOUPLED (the integrator terms live there; a bare QuadEnv raises AttributeError in the reference): QR_E_KIND otherwise.
 * Same side effect on the integrators. */
int qr_error_obs_format(const QrEnv* env, int32_t format, float* obs0, float* obs1, void* stream);

/* Replaces QuadEnv.reset(env_type) (quad.py:171-222, 338-404) for every env with
 * mask[i] != 0 (mask NULL = all): draws UDM parameters (unless QR_FLAG_NO_UDM / no params
 * buffer), the initial error state, R = Rz(yaw)Ry(pitch)Rx(roll), zeroes the integrators
 * and step counters and bumps the episode counter.  Counter-based Philox4x32-10 keyed by
 * (seed, env_offset+i, episode): results do not depend on sharding or launch geometry. */
int qr_reset(const QrEnv* env, const uint8_t* mask, void* stream);

/* Replaces QuadEnv.get_current_state() (quad.py:409-410): writes the reference's float64
 * 18-vector rows [N][18] = (x, v, vec_F(R(q)), W). */
int qr_get_state(const QrEnv* env, double* rows, void* stream);

/* Replaces assignment to QuadEnv.state: reads float64 rows [N][18] for envs with
 * mask[i] != 0 (NULL = all).  R is first passed through the reference's ensure_SO3 rule
 * (quad_utils.py:123-142) — and, because the internal attitude is a unit quaternion, always
 * projected onto SO(3) (nearest rotation, the same U V^T the reference's SVD yields).
 * A row whose attitude block has det R <= 0 or a non-finite entry has no nearest rotation: it is
 * REJECTED (that env keeps its previous state) and counted in *rejected (device int32, optional,
 * zero it before the call; the host wrapper raises when it is non-zero). */
int qr_set_state(const QrEnv* env, const double* rows, const uint8_t* mask, int32_t* rejected, void* stream);

/* Dry run of qr_set_state: counts in *rejected (device int32, required, zero it before the call) the rows qr_set_state would
 * reject — the same test on the same data — and writes NOTHING.  Lets a caller that injects states together with other
 * per-env data (integrator terms, parameters) refuse the whole injection before any of it is applied. */
int qr_check_state(const QrEnv* env, const double* rows, const uint8_t* mask, int32_t* rejected, void* stream);

/* Replaces TrajectoryGenerator.mark_traj_start(state) (utils/trajectory_generator.py:176-204)
 * plus the episode-start branch of calculate_desired (mode 0 :141-148: b1d = Rz(theta) b1_proj,
 * theta ~ U(+-25 deg); mode 1 :253-266: x_init, t_traj ~ U(2,5) s, w_b1d ~ U(+-0.15 pi) rad/s)
 * for envs with mask[i] != 0 (NULL = all), from the CURRENT state.  `draws` (optional, device,
 * [3][N] = theta_b1d [rad], t_traj [s], w_b1d [rad/s]) injects the random draws; NULL draws them
 * from the env's Philox stream.  Requires env->traj and goal_mode != QR_GOAL_EXTERNAL. */
int qr_traj_start(const QrEnv* env, const uint8_t* mask, const float* draws, void* stream);

/* Replaces TrajectoryGenerator.get_desired(state, mode) (trajectory_generator.py:113-173) for
 * the CURRENT state of envs with mask[i] != 0 (NULL = all): advances the per-env call counter
 * (t += dt) and writes rows [N][15] = (xd, vd, b1d, b1d_dot, Wd), Wd = (0, 0, b3 . (b1c x b1c_dot)) (:165-172).  With
 * store_goal != 0 the result also becomes the env's goal buffer (set_goal_state).  The fused
 * path (goal_mode != QR_GOAL_EXTERNAL in qr_step / qr_rollout) does the same at the start of every env-step
 * and after an in-launch reset, exactly as main.py:145-147,226-229 call it. */
int qr_get_desired(const QrEnv* env, const uint8_t* mask, float* rows, int32_t store_goal, void* stream);

/* Replaces the GAE loop of the reference's PPO (algos/ppo/ppo.py:134-146) for a [T][M] rollout
 * (M = num_envs * n_agents columns, each an independent time series):
 *     delta_t = r_t + gamma * Vnext_t * (1 - done_t) - V_t
 *     A_t     = delta_t + gamma * lambda * (1 - done_t) * A_{t+1},   A_T = 0   (reverse scan)
 *     target_t = A_t + V_t
 *   reward [T][M] f32, done [T][M] u8, value [T][M] f32 (or [T+1][M] when next_value is NULL:
 *   then Vnext_t = value[t+1], row T being the bootstrap value), next_value [T][M] f32 or NULL.
 *   Outputs advantage, td_target [T][M] f32 and, if `partials` != NULL, per-workgroup
 *   (sum, sum of squares) of the advantages as double [grid][2] (grid = ceil(M/64)) for the
 *   normalisation (adv - mean)/(std + 1e-4) (ppo.py:147); summing them on the host side of the
 *   launch is deterministic (no atomics). */
int qr_gae(const float* reward, const uint8_t* done, const float* value, const float* next_value,
           int32_t n_steps, int64_t n_cols, float gamma, float lam,
           float* advantage, float* td_target, double* partials, void* stream);

/* The reference's MLP critics for a whole PPO horizon, between the collection launch and qr_gae:
 *     v = fc3(tanh(fc2(tanh(fc1(x)))))        MLP_Critic / MLP_Critic_CTDE, algos/ppo/ppo_mlp.py:64-126
 * on float32 AoS rows, weights in torch.nn.Linear layout, used in place.  The input row x is the first in0 columns of the
 * obs0 row followed by the first in1 columns of the obs1 row (MLP_Critic_CTDE's torch.cat); in0 / in1 are 0 or the full
 * width of that row tensor, which is also its row stride.  1 <= in0 + in1 <= 24, 1 <= hidden_dim <= 64. */
typedef struct QrCritic {
  const float *fc1_w, *fc1_b;       /* [hidden][in0+in1], [hidden] */
  const float *fc2_w, *fc2_b;       /* [hidden][hidden],  [hidden] */
  const float *fc3_w, *fc3_b;       /* [1][hidden], [1]            */
  int32_t in0, in1;                 /* columns taken from the obs0 / obs1 rows: 0 or the full row width */
  int32_t hidden_dim, reserved0;
} QrCritic;
/* value[i * value_stride] = V(row i) for i < n_rows — agent k's critic writes column k of a [.., n_agents] tensor with
 * value = base + k, value_stride = n_agents.  One launch; n_rows = 0 launches nothing.  QR_E_NULL for a NULL critic, weight or
 * value pointer, or a NULL row pointer whose in0 / in1 is not 0; QR_E_SIZE for sizes outside the ranges above, n_rows < 0 or
 * value_stride < 1; QR_E_ALIGN for a float pointer that is not 4-byte aligned. */
int qr_critic_values(const QrCritic* critic, const float* obs0, const float* obs1, int64_t n_rows,
                     float* value, int32_t value_stride, void* stream);
/* The reference's V(obs_next) (ppo.py:128-131) for the [T][N] transitions of an auto-resetting env, one launch:
 *     next_value[t][n] = reset(t, n) ? V(final_obs[t][n]) : value[t+1][n],   reset = any of done[t][n][0..n_agents) or truncated[t][n]
 * value is [T+1][N] (row t+1 = V of the observation after step t, filled by the call above), next_value [T][N], both with element
 * stride value_stride; final_obs0 / final_obs1 [T][N][in0 / in1] (QrStepOut.final_obs*), done [T][N][n_agents], truncated [T][N] or
 * NULL.  The choice is a select: rows of final_obs of envs that did not reset are never used, whatever they hold.  Errors as
 * above, and QR_E_SIZE for n_steps < 1, n_envs < 0 or n_agents < 1; n_envs = 0 launches nothing. */
int qr_critic_next_values(const QrCritic* critic, const float* final_obs0, const float* final_obs1,
                          const uint8_t* done, int32_t n_agents, const uint8_t* truncated,
                          int32_t n_steps, int64_t n_envs, const float* value, float* next_value,
                          int32_t value_stride, void* stream);

/* The actor half of one PPO minibatch update (PPO.train, algos/ppo/ppo.py:169-182, with algos/policy_regularization.py) for ONE
 * agent, read from the rollout storage in place: loss and gradients with respect to the actor's seven tensors, without autograd.
 * A row i of the minibatch is an index into the flat [T * N] transitions (i = t N + n):
 *     mu    = actor(obs[i]) (QR_ACTOR_TANH_MEAN form, log_std parameter s)      lp_j = Normal(mu_j, exp(s_j)).log_prob(action[i][j])
 *     rho   = exp(sum_j lp_j - sum_j logp_old[i][j])          S = min(rho adv_i, clamp(rho, 1 - clip, 1 + clip) adv_i)
 *     loss  = -(1/B) sum_i (S_i + entropy_coef sum_j (0.5 + 0.5 log 2 pi + s_j))
 *             + lam_T mean (c(mu(obs[i])) - c(mu(obs_next[i])))^2 + lam_S mean (c(mu(obs[i])) - c(mu(obs[i] + noise)))^2
 *             + lam_M mean (c(mu(obs[i])) - nominal)^2,         c = clamp to +-max_action, means over the B x action_dim elements
 * obs_next[i] = final_obs[i] where any of done[i][0..n_agents) or truncated[i] is set, obs[i + N] elsewhere (qr_critic_next_values'
 * rule; final_obs NULL: always obs[i + N], done / truncated unread).  The gradients are torch autograd's: min and clamp route
 * them as torch.min / torch.clamp do.  A coefficient lam_* equal to 0 skips that term's passes.
 *   obs [T+1][N][obs_dim], final_obs [T][N][obs_dim]; action / logp_old: row i at base + i * row_stride + col_offset (the
 *   Decoupled storage's [T][N][5] rows serve both agents); advantage: element i at advantage[i * adv_stride]; index: int64
 *   [batch] or NULL (rows 0 .. batch - 1; repeats are legal, a value outside [0, T N) is clamped into it); noise [obs_dim]
 *   (required when lam_S != 0), nominal [action_dim] (required when lam_M != 0).
 * Two launches: one wavefront per workgroup accumulates its share of the 64-row tiles and writes ONE partial vector into
 * `workspace`; a second kernel sums the partial vectors in float64 in a fixed order.  The same inputs and grid give the same
 * bits (no atomics).  The grid is min(ceil(batch / 64), max_workgroups), max_workgroups = 0: the library's rule (1024). */
typedef struct QrPpoBatch {
  const float* obs;        const float* final_obs;
  const uint8_t* done;     const uint8_t* truncated;
  const float* action;     const float* logp_old;
  const float* advantage;
  const int64_t* index;
  const float* noise;      const float* nominal;
  void* workspace;         int64_t workspace_bytes;   /* >= qr_ppo_actor_workspace_bytes(...); 8-byte aligned */
  int64_t batch, n_envs;                              /* B >= 1; N */
  int32_t n_steps, n_agents;                          /* T; columns of done */
  int32_t row_stride, col_offset;                     /* of the action and logp_old rows */
  int32_t adv_stride, max_workgroups;
  float clip, entropy_coef, lam_T, lam_S, lam_M, max_action;
} QrPpoBatch;
/* Outputs, overwritten: the gradient tensors in the shapes of the QrActor's (log_std [action_dim]) and stats [4] = loss, mean S_i,
 * share of rows with rho outside [1 - clip, 1 + clip], mean of (rho - 1) - log rho. */
typedef struct QrPpoGrad {
  float *fc1_w, *fc1_b, *fc2_w, *fc2_b, *mean_w, *mean_b, *log_std, *stats;
} QrPpoGrad;
/* QR_E_NULL for a NULL struct, weight, input, output or workspace pointer (final_obs, truncated, index optional; done required
 * with final_obs; noise / nominal as above); QR_E_KIND for squash != QR_ACTOR_TANH_MEAN or an actor with a log_std head;
 * QR_E_SIZE for sizes other than qr_rollout_actor's (23,16,4), (15,16,4), (3,4,1), batch < 1, n_steps < 1, n_envs < 1, strides
 * < 1, a column offset outside the row, max_workgroups < 0 or a workspace that is too small; QR_E_ALIGN for a float pointer that is
 * not 4-byte aligned or an index / workspace pointer that is not 8-byte aligned.  Nothing is launched on an error. */
int qr_ppo_actor_grad(const QrActor* actor, const QrPpoBatch* batch, const QrPpoGrad* grad, void* stream);
/* The same with the entropy coefficient in device memory: entropy_coef_dev not NULL — the reduce launch READS the coefficient from that
 * float (it is never written) and batch->entropy_coef is ignored, so that a recorded launch follows a coefficient that decays between
 * replays; with the word holding c the result is, bit for bit, qr_ppo_actor_grad's with entropy_coef = c.  NULL: qr_ppo_actor_grad
 * itself.  The errors are that entry's, and QR_E_ALIGN for an entropy_coef_dev that is not 4-byte aligned. */
int qr_ppo_actor_grad_dev(const QrActor* actor, const QrPpoBatch* batch, const QrPpoGrad* grad, const float* entropy_coef_dev, void* stream);
/* Bytes of workspace qr_ppo_actor_grad needs for this actor size, batch and max_workgroups; QR_E_SIZE (< 0) where it would refuse them. */
int64_t qr_ppo_actor_workspace_bytes(int32_t obs_dim, int32_t hidden_dim, int32_t action_dim, int64_t batch, int32_t max_workgroups);

/* The critic half of one PPO minibatch update (PPO.train, algos/ppo/ppo.py:193-214) for ONE critic (a QrCritic as above: MLP_Critic
 * or MLP_Critic_CTDE, 1 <= in0 + in1 <= 24, 1 <= hidden_dim <= 64), read from the rollout storage in place: loss and gradients with
 * respect to the critic's six tensors, without autograd.  A row i of the minibatch is an index into the observation rows:
 *     v_i   = V(x_i)             x_i = obs0 row index[i] (CTDE: followed by obs1 row index[i])
 *     e_i   = v_i - y_i          y_i = target[index[i] * target_stride]
 *     mse   = (1/B) sum_i e_i^2
 *     loss  = mse + l2_reg (||fc1_w||^2 + ||fc2_w||^2 + ||fc3_w||^2)          (ppo.py:197-204: the weights, not the biases)
 * The gradients are loss.backward()'s: the data term backwards from dLoss/dv_i = 2 e_i / B, plus 2 l2_reg W on the three weights.
 *   obs0 / obs1: float32 rows [>= rows][in0 / in1] (NULL where in0 / in1 is 0); target: element i at target[i * target_stride], i <
 *   rows (the storage's td_target column of this agent); index: int64 [batch] or NULL (rows 0 .. batch - 1; repeats are legal, a
 *   value outside [0, rows) is clamped into it).
 * Two launches: one wavefront per workgroup accumulates its share of the 64-row tiles and writes ONE partial vector into
 * `workspace`; a second kernel sums the partial vectors in float64 in a fixed order and adds the L2 terms.  The same inputs and grid
 * give the same bits (no atomics).  The grid is min(ceil(batch / 64), max_workgroups), max_workgroups = 0: the library's rule (1024). */
typedef struct QrCriticBatch {
  const float* obs0;       const float* obs1;
  const float* target;
  const int64_t* index;
  void* workspace;         int64_t workspace_bytes;   /* >= qr_ppo_critic_workspace_bytes(...); 8-byte aligned */
  int64_t batch, rows;                                /* B >= 1; rows of obs0 / obs1 and elements of target an index may name */
  int32_t target_stride, max_workgroups;
  float l2_reg;            int32_t reserved0;
} QrCriticBatch;
/* Outputs, overwritten: the gradient tensors in the shapes of the QrCritic's and stats [4] = loss, mse, mean of e_i, population
 * variance of y_i over the minibatch (explained variance = 1 - (stats[1] - stats[2]^2) / stats[3]: the division is the caller's, so
 * that a constant target puts no NaN into the output). */
typedef struct QrCriticGrad {
  float *fc1_w, *fc1_b, *fc2_w, *fc2_b, *fc3_w, *fc3_b, *stats;
} QrCriticGrad;
/* QR_E_NULL for a NULL struct, weight, target, output or workspace pointer, or a NULL row pointer whose in0 / in1 is not 0 (index
 * optional); QR_E_SIZE for widths outside the ranges above, batch < 1, rows < 1, target_stride < 1, max_workgroups < 0 or a workspace
 * that is too small; QR_E_ALIGN for a float pointer that is not 4-byte aligned or an index / workspace pointer that is not 8-byte
 * aligned.  Nothing is launched on an error. */
int qr_ppo_critic_grad(const QrCritic* critic, const QrCriticBatch* batch, const QrCriticGrad* grad, void* stream);
/* Bytes of workspace qr_ppo_critic_grad needs for this critic size (in_dim = in0 + in1), batch and max_workgroups; QR_E_SIZE (< 0)
 * where it would refuse them. */
int64_t qr_ppo_critic_workspace_bytes(int32_t in_dim, int32_t hidden_dim, int64_t batch, int32_t max_workgroups);

/* What follows each gradient launch in PPO.train (algos/ppo/ppo.py:185-190, 209-214) — torch.nn.utils.clip_grad_norm_,
 * torch.optim.AdamW.step() (amsgrad = False, maximize = False) and CosineAnnealingWarmRestarts(T_0, eta_min).step() — for up to 8
 * independent parameter groups in ONE launch, one workgroup per group.  A group is what one AdamW instance holds: an actor's seven
 * tensors, a critic's six.  With t = *step + 1:
 *     total_norm = the 2-norm over all of the group's gradient entries (float64 sums in a fixed order)
 *     lr_t       = eta_min + (lr - eta_min) (1 + cos(pi ((t - 1) mod t0) / t0)) / 2     (t0 = 0: lr_t = lr) — the scheduler is stepped
 *                  AFTER the optimiser, so the t-th optimiser step sees eta(t - 1)
 *     clip_coef  = min(1, max_norm / (total_norm + 1e-6))                               (max_norm < 0: 1, clipping is off)
 *     g = clip_coef grad;  p *= 1 - lr_t weight_decay;  m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g^2
 *     p -= (lr_t / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 * the scalars in float64, the per-entry arithmetic in float32.  Parameters, exp_avg, exp_avg_sq and *step are updated in place;
 * stats [4] = total_norm, clip_coef, lr_t, t.  The GRADIENT tensors are read only: unlike clip_grad_norm_, which scales .grad in
 * place, they keep the unclipped gradient.  Non-finite gradients propagate (error_if_nonfinite = False).  No atomics: equal inputs
 * give equal bits.  Groups must not share memory. */
typedef struct QrAdamWGroup {
  float* param[8];  const float* grad[8];  int32_t count[8];  int32_t n_tensors;   /* 1..8 tensors, count >= 1 each */
  float* exp_avg;   float* exp_avg_sq;     /* [sum of count] each, the tensors back to back; zero before the first step */
  int64_t* step;                            /* device: steps taken so far */
  float* stats;                             /* device [4] or NULL */
  double lr, eta_min;  int64_t t0;          /* base rate; schedule (t0 = 0: constant) */
  float beta1, beta2, eps, weight_decay, max_norm;   /* max_norm < 0: no clipping */
} QrAdamWGroup;
/* QR_E_NULL for a NULL struct, param, grad, state or step pointer (stats optional); QR_E_SIZE for n_groups outside 1..8, n_tensors
 * outside 1..8, a count < 1, a group of more than 65 536 entries, lr / eta_min / eps / weight_decay negative or not finite, a beta
 * outside [0, 1), t0 < 0 or a NaN max_norm; QR_E_ALIGN for a float pointer that is not 4-byte aligned or a step pointer that is not
 * 8-byte aligned.  Nothing is launched on an error. */
int qr_adamw_step(const QrAdamWGroup* groups, int32_t n_groups, void* stream);

/* qr_adamw_step for groups of up to 16 tensors, with what TD3.train / SAC.train do right after the optimiser step fused into the same
 * launch — up to 7 independent groups, one workgroup each (7 descriptors of 552 bytes fit one 4 096-byte kernarg segment, 8 do not).
 * Sixteen slots hold the reference's twin critic (twelve tensors) as ONE group: one clip_grad_norm_ over all twelve and one step
 * counter, as torch.optim.AdamW(critic.parameters()) has them (td3.py:166-171, sac.py:165-170).  The step itself is qr_adamw_step's,
 * arithmetic, order and stats: a group of at most 8 tensors with no target and no exp_out gets the bits of qr_adamw_step.  Then
 *     target[k][i] = fl(fl(tau32 * param[k][i]) + fl(omt32 * target[k][i]))   for every k with target[k] != NULL, from the NEW param[k]
 * — qr_soft_update's expression and rounding, so the bits of qr_soft_update(param[k], target[k], tau) run after the step
 * (td3.py:207-211, sac.py:219-221); target[k] = NULL leaves tensor k without one, all NULL is a plain step — and
 *     *exp_out = float32(exp(float64(param[0][0])))                           where exp_out != NULL, from the NEW value
 * for a group of exactly one entry: SAC's alpha = log_alpha.exp() (sac.py:213).  Targets and exp_out are written by the thread that
 * wrote the parameter entry; groups, and the tensors of a group, must not share memory.  reserved0 must be 0. */
typedef struct QrAdamWPolyakGroup {
  float* param[16];  const float* grad[16];  float* target[16];   /* target[k]: NULL or [count[k]] */
  int32_t count[16];  int32_t n_tensors, reserved0;               /* 1..16 tensors, count >= 1 each; 0 */
  float* exp_avg;   float* exp_avg_sq;     /* [sum of count] each, the tensors back to back; zero before the first step */
  int64_t* step;                            /* device: steps taken so far */
  float* stats;                             /* device [4] or NULL */
  float* exp_out;                           /* device [1] or NULL; only with one tensor of one entry */
  double lr, eta_min;  int64_t t0;          /* base rate; schedule (t0 = 0: constant) */
  float beta1, beta2, eps, weight_decay, max_norm;   /* max_norm < 0: no clipping */
  double tau;                               /* in [0, 1]; read only where a target is set, checked always */
} QrAdamWPolyakGroup;
/* QR_E_NULL for a NULL struct, param, grad, state or step pointer (stats, exp_out and every target optional); QR_E_SIZE for n_groups
 * outside 1..7, n_tensors outside 1..16, reserved0 != 0, a count < 1, a group of more than 65 536 entries, lr / eta_min / eps /
 * weight_decay negative or not finite, a beta outside [0, 1), t0 < 0, a NaN max_norm, tau outside [0, 1] or not finite, exp_out on a
 * group of more than one entry, or a target pointer equal to its param pointer; QR_E_ALIGN for a float pointer that is not 4-byte
 * aligned or a step pointer that is not 8-byte aligned.  Nothing is launched on an error. */
int qr_adamw_polyak_step(const QrAdamWPolyakGroup* groups, int32_t n_groups, void* stream);

/* The critic half of one TD3 minibatch update (TD3.train, algos/td3/td3.py:123-167, the non-CTDE branch) for ONE agent, read from a
 * flat transition buffer in place, without autograd.  The reference's twin critic MLP_Critic (algos/td3/td3_mlp.py:36-99), twelve
 * float32 tensors in torch.nn.Linear layout, used in place:
 *     Q1 = fc3(relu(fc2(relu(fc1(sa)))))     Q2 = fc6(relu(fc5(relu(fc4(sa)))))     sa = the observation row followed by the action row
 * obs_dim >= 1, action_dim >= 1, obs_dim + action_dim <= 28, 1 <= hidden_dim <= 64.  reserved0 must be 0.  The centralized (CTDE)
 * critic, whose rows come from four sources, is this struct too, with the summed widths: the sources are QrCtdeTransitions', below. */
typedef struct QrQCritic {
  const float *fc1_w, *fc1_b;       /* [hidden][obs_dim+action_dim], [hidden]     Q1 */
  const float *fc2_w, *fc2_b;       /* [hidden][hidden], [hidden]                    */
  const float *fc3_w, *fc3_b;       /* [1][hidden], [1]                              */
  const float *fc4_w, *fc4_b;       /* as fc1                                     Q2 */
  const float *fc5_w, *fc5_b;       /* as fc2                                        */
  const float *fc6_w, *fc6_b;       /* as fc3                                        */
  int32_t obs_dim, action_dim;
  int32_t hidden_dim, reserved0;
} QrQCritic;
/* What the reference's ReplayBuffer (algos/replay_buffer.py) holds for one agent, as flat float32 tensors, and one minibatch of it:
 *   obs, obs_next [>= rows][obs_dim]; action: row i at action + i * row_stride + col_offset (as in QrPpoBatch); reward, done: element
 *   i at reward[i * reward_stride], done[i * done_stride] (done is 0.0 or 1.0); index: int64 [batch] or NULL (rows 0 .. batch - 1;
 *   repeats are legal, a value outside [0, rows) is clamped into it).  A pointer the entry point does not read may be NULL:
 *   qr_twinq_target reads obs_next, reward, done and index; qr_twinq_grad reads obs, action and index. */
typedef struct QrTransitions {
  const float* obs;        const float* obs_next;
  const float* action;
  const float* reward;     const float* done;
  const int64_t* index;
  int64_t batch, rows;                                /* B >= 1; rows an index may name */
  int32_t row_stride, col_offset;                     /* of the action rows */
  int32_t reward_stride, done_stride;
} QrTransitions;
/* The TD3 target of a minibatch in ONE launch (td3.py:139-154), j the minibatch position and i = index[j]:
 *     a'_j = clamp(pi_targ(obs_next[i]) + clamp(target_noise * eps[j], +-noise_clip), +-max_action)
 *     y[j] = reward[i] + discount * (1 - done[i]) * min(Q1_targ, Q2_targ)(obs_next[i], a'_j)
 * pi_targ: a QrActor of the QR_ACTOR_TANH_MEAN form (MLP_Actor_TD3: tanh(fc3(relu(fc2(relu(fc1(x))))))) in one of
 * qr_ppo_actor_grad's three sizes, its obs_dim and action_dim equal to the critic's; its log_std is not read.  eps: [batch][action_dim]
 * float32 standard-normal draws, row j for minibatch position j (not for index[j]); NULL: no smoothing noise, the same bits as
 * zeros.  actor_target NULL: a'_j = action_next[j] ([batch][action_dim], used as it is: eps and the clamps do not apply) — the
 * next action of another policy form (SAC's sample), or a critic wider than any actor this library holds.  A row with done = 1 gets
 * y = reward exactly (for finite Q).  Only the rows the index names are read.  y: [batch] float32, plain stores. */
typedef struct QrTd3Target {
  const float* eps;
  const float* action_next;
  float* y;
  float discount, target_noise, noise_clip, max_action;
} QrTd3Target;
/* QR_E_NULL for a NULL critic, batch or target struct, weight, obs_next, reward, done or y pointer, or actor_target and action_next
 * both NULL; QR_E_KIND for an actor with squash != QR_ACTOR_TANH_MEAN or a log_std head; QR_E_SIZE for widths outside the ranges
 * above, reserved0 != 0, an actor size other than (23,16,4), (15,16,4), (3,4,1), an actor whose obs_dim or action_dim differs from
 * the critic's, batch < 1, rows < 1, a stride < 1 or a negative or non-finite noise_clip / max_action; QR_E_ALIGN for a float pointer
 * that is not 4-byte aligned or an index pointer that is not 8-byte aligned.  Nothing is launched on an error. */
int qr_twinq_target(const QrActor* actor_target, const QrQCritic* critic_target, const QrTransitions* batch, const QrTd3Target* target,
                  void* stream);
/* The twin-Q regression against a given target (td3.py:157-167 without the equivariant term; SAC's critic update has the same form):
 *     loss = (1/B) sum_j (Q1(obs[i], action[i]) - y[j])^2 + (1/B) sum_j (Q2(obs[i], action[i]) - y[j])^2,      i = index[j]
 * and loss.backward()'s gradients for the twelve tensors.  y: [batch] float32 by minibatch position (qr_twinq_target's output).
 * Outputs, overwritten: the gradient tensors in the shapes of the QrQCritic's and stats [4] = loss, the Q1 mse, the Q2 mse, the
 * mean of y.  Two launches: one wavefront per workgroup owns ONE of the two networks, accumulates its share of the 64-row tiles and
 * writes ONE partial vector into `workspace`; a second kernel sums the partial vectors in float64 in a fixed order.  The same inputs
 * and grid give the same bits (no atomics).  The grid is 2 x min(ceil(batch / 64), max_workgroups), max_workgroups = 0: the
 * library's rule (512 per network). */
typedef struct QrTwinQGrad {
  float *fc1_w, *fc1_b, *fc2_w, *fc2_b, *fc3_w, *fc3_b, *fc4_w, *fc4_b, *fc5_w, *fc5_b, *fc6_w, *fc6_b, *stats;
  const float* y;
  void* workspace;         int64_t workspace_bytes;   /* >= qr_twinq_workspace_bytes(...); 8-byte aligned */
  int32_t max_workgroups, reserved0;
} QrTwinQGrad;
/* QR_E_NULL for a NULL struct, weight, obs, action, y, output or workspace pointer (index optional); QR_E_SIZE for widths outside
 * the ranges above, reserved0 != 0, batch < 1, rows < 1, row_stride < 1, a column offset outside the row, max_workgroups < 0 or a
 * workspace that is too small; QR_E_ALIGN for a float pointer that is not 4-byte aligned or an index / workspace pointer that is not
 * 8-byte aligned.  Nothing is launched on an error. */
int qr_twinq_grad(const QrQCritic* critic, const QrTransitions* batch, const QrTwinQGrad* grad, void* stream);
/* Bytes of workspace qr_twinq_grad needs for this critic size (in_dim = obs_dim + action_dim), batch and max_workgroups; QR_E_SIZE
 * (< 0) where it would refuse them. */
int64_t qr_twinq_workspace_bytes(int32_t in_dim, int32_t hidden_dim, int64_t batch, int32_t max_workgroups);

/* The actor half of one TD3 minibatch update (TD3.train, algos/td3/td3.py:177-196, the non-CTDE branch without the equivariant
 * term, with algos/policy_regularization.py) for ONE agent, read from the transition buffer in place: the loss and loss.backward()'s
 * gradients with respect to the actor's six tensors, without autograd.  With j the minibatch position and i = index[j]:
 *     a_j     = clamp(pi(obs[i]), +-max_action)              pi = tanh(fc3(relu(fc2(relu(fc1 x)))))     (MLP_Actor_TD3)
 *     a_next  = clamp(pi(obs_next[i]), +-max_action)
 *     a_pert  = clamp(pi(obs[i] + noise), +-max_action)      noise: ONE [obs_dim] row, broadcast
 *     loss    = -(1/B) sum_j Q1(obs[i], a_j) + lam_T mse(a, a_next) + lam_S mse(a, a_pert) + lam_M mse(a, nominal)
 * mse: the mean over the B x action_dim elements.  The gradients flow through all three evaluations of pi (neither a_next nor a_pert
 * is detached) and through Q1 into a; the critic's own gradients are not produced.  clamp routes a gradient where |pi| <= max_action,
 * as torch.clamp does.  A coefficient lam_* equal to 0 skips that term's passes.
 *   actor: a QrActor of the QR_ACTOR_TANH_MEAN form in one of the sizes (23,16,4), (15,16,4), (3,4,1); its log_std is not read.
 *   critic: a QrQCritic as above whose obs_dim and action_dim equal the actor's; only fc1 .. fc3 (Q1) are read, fc4 .. fc6 may be NULL.
 *   batch: obs, obs_next (read only with lam_T != 0) and index of a QrTransitions (index: int64 [batch] or NULL; repeats are legal, a
 *   value outside [0, rows) is clamped into it).  noise [obs_dim]: required when lam_S != 0; nominal [action_dim]: when lam_M != 0.
 * Outputs, overwritten: the six gradient tensors in the shapes of the QrActor's and stats [4] = loss, the mean of Q1(obs, a), the share
 * of the B x action_dim components of pi(obs) with |pi| > max_action (an exact count over B x action_dim), and
 * lam_T L_T + lam_S L_S + lam_M L_M.
 * Two launches: one wavefront per workgroup accumulates its share of the 64-row tiles and writes ONE partial vector into `workspace`;
 * a second kernel sums the partial vectors in float64 in a fixed order.  The same inputs and grid give the same bits (no atomics).
 * The grid is min(ceil(batch / 64), max_workgroups), max_workgroups = 0: the library's rule (1024). */
typedef struct QrDpgGrad {
  float *fc1_w, *fc1_b, *fc2_w, *fc2_b, *mean_w, *mean_b, *stats;
  const float* noise;      const float* nominal;
  void* workspace;         int64_t workspace_bytes;   /* >= qr_dpg_actor_workspace_bytes(...); 8-byte aligned */
  float lam_T, lam_S, lam_M, max_action;
  int32_t max_workgroups, reserved0;
} QrDpgGrad;
/* QR_E_NULL for a NULL struct, actor weight, Q1 weight, obs, output or workspace pointer (index optional; obs_next, noise, nominal as
 * above); QR_E_KIND for squash != QR_ACTOR_TANH_MEAN or an actor with a log_std head; QR_E_SIZE for an actor size other than the
 * three above, critic widths outside their ranges, an actor whose obs_dim or action_dim differs from the critic's, reserved0 != 0
 * (either struct), batch < 1, rows < 1, max_workgroups < 0, a negative or non-finite max_action or lam_*, or a workspace that is too
 * small; QR_E_ALIGN for a float pointer that is not 4-byte aligned or an index / workspace pointer that is not 8-byte aligned.
 * Nothing is launched on an error. */
int qr_dpg_actor_grad(const QrActor* actor, const QrQCritic* critic, const QrTransitions* batch, const QrDpgGrad* grad, void* stream);
/* Bytes of workspace qr_dpg_actor_grad needs for this actor size, critic width, batch and max_workgroups; QR_E_SIZE (< 0) where it
 * would refuse them. */
int64_t qr_dpg_actor_workspace_bytes(int32_t obs_dim, int32_t hidden_dim, int32_t action_dim, int32_t critic_hidden_dim, int64_t batch,
                                     int32_t max_workgroups);

/* The soft (Polyak) target update of TD3.train (td3.py:207-211) for up to 24 tensors in ONE launch — a twin critic's twelve and an
 * actor's six with room to spare:
 *     target[k][i] = fl(fl(tau32 * param[k][i]) + fl(omt32 * target[k][i])),   tau32 = float32(tau), omt32 = float32(1.0 - tau)
 * float32 in torch's order, every operation rounded on its own (no fused multiply-add), the subtraction 1.0 - tau in double: the bits
 * of `target_param.data.copy_(tau * param.data + (1 - tau) * target_param.data)`.  In place on `target`; `param` is read only.
 * Tensors must not overlap. */
typedef struct QrSoftUpdate {
  float* target[24];  const float* param[24];  int64_t count[24];   /* entries of each tensor, >= 1 */
  int32_t n_tensors, reserved0;                                     /* 1..24; 0 */
  double tau;                                                       /* in [0, 1] */
} QrSoftUpdate;
/* QR_E_NULL for a NULL struct, target or param pointer; QR_E_SIZE for n_tensors outside 1..24, reserved0 != 0, a count < 1, tau
 * outside [0, 1] or not finite, or a target pointer equal to its param pointer; QR_E_ALIGN for a pointer that is not 4-byte aligned.
 * Nothing is launched on an error. */
int qr_soft_update(const QrSoftUpdate* update, void* stream);

/* SAC's soft target values of a minibatch in ONE launch (SAC.train, algos/sac/sac.py:135-153, the non-CTDE branch, with
 * MLP_Actor_SAC.sample, algos/sac/sac_mlp.py:55-79), j the minibatch position and i = index[j]:
 *     mean, ls = pi(obs_next[i]);   ls = clamp(ls, -20, 2)                     pi: the LIVE actor (SAC has no target actor)
 *     u = mean + exp(ls) * eps[j];  a'_j = tanh(u)
 *     logp_j = sum_f [ -eps[j][f]^2 / 2 - ls_f - log sqrt(2 pi) - log(1 - a'_f^2 + 1e-6) ]
 *     y[j] = reward[i] + discount * (1 - done[i]) * ( min(Q1_targ, Q2_targ)(obs_next[i], a'_j) - alpha * logp_j )
 * 1 - a'^2 is formed as 4 t / (1 + t)^2 and a' as copysign((1 - t) / (1 + t), u) with t = exp(-2 |u|), not from the rounded a': the
 * same function without the cancellation, good to a relative 1e-6 at every |u|.  -eps^2 / 2 is formed from eps directly, not as
 * -(u - mean)^2 / (2 var).
 * actor: a QrActor of the QR_ACTOR_TANH_SAMPLE form with the log_std head (MLP_Actor_SAC: fc1, fc2, mean_linear, log_std_linear) in one
 * of qr_twinq_target's three sizes, its obs_dim and action_dim equal to the critic's; its log_std member is not read.  eps:
 * [batch][action_dim] float32 standard-normal draws (rsample's), row j for minibatch position j (not for index[j]); NULL: zeros, the
 * same bits as zeros.  alpha: the entropy temperature; alpha_dev, where not NULL, is a device float that is read in the kernel and
 * wins (the reference's sac_alpha is a device tensor under automatic entropy tuning: the host never synchronises for it).
 * actor NULL: a'_j = action_next[j] ([batch][action_dim]) and logp_j = logp_next[j] ([batch]) are used as they are — another policy
 * form, or a critic wider than any actor this library holds; eps is not read.  action_out [batch][action_dim] and logp_out [batch]:
 * optional, a'_j and logp_j as used; giving them or not changes no bit of y.  A row with done = 1 gets y = reward exactly (for finite
 * Q and logp).  Only the rows the index names are read.  y: [batch] float32.  Plain stores, no atomics: equal inputs give equal bits.
 * The grid is qr_twinq_target's. */
typedef struct QrSacTarget {
  const float* eps;
  const float* action_next;  const float* logp_next;
  const float* alpha_dev;
  float* y;
  float* action_out;         float* logp_out;
  float discount, alpha;
} QrSacTarget;
/* QR_E_NULL for a NULL critic, batch or target struct, weight, obs_next, reward, done or y pointer, or an actor of NULL with
 * action_next or logp_next NULL; QR_E_KIND for an actor with squash != QR_ACTOR_TANH_SAMPLE or without the log_std head; QR_E_SIZE for
 * widths outside QrQCritic's ranges, reserved0 != 0, an actor size other than (23,16,4), (15,16,4), (3,4,1), an actor whose obs_dim or
 * action_dim differs from the critic's, batch < 1, rows < 1, a stride < 1 or a negative or non-finite discount or alpha; QR_E_ALIGN
 * for a float pointer that is not 4-byte aligned or an index pointer that is not 8-byte aligned.  Nothing is launched on an error. */
int qr_sac_target(const QrActor* actor, const QrQCritic* critic_target, const QrTransitions* batch, const QrSacTarget* target, void* stream);

/* The actor half of one SAC minibatch update (SAC.train, algos/sac/sac.py:182-211, the non-CTDE branch without the spectral-norm
 * term, with algos/policy_regularization.py for rl_algo == "SAC" and MLP_Actor_SAC.sample, algos/sac/sac_mlp.py:55-79) for ONE agent,
 * read from the transition buffer in place: the loss, loss.backward()'s gradients with respect to the actor's eight tensors and what
 * alpha's own update needs, without autograd.  With j the minibatch position, i = index[j] and c(.) the clamp to +-max_action:
 *     sample(x, e):  mean, ls = pi(x);  ls = clamp(ls, -20, 2);  u = mean + exp(ls) * e;  a = tanh(u)
 *                    logp = sum_f [ -e^2 / 2 - ls - log sqrt(2 pi) - log(1 - a^2 + 1e-6) ]
 *     loss pass:     (a, logp) = sample(obs[i], eps[j])                              (no clamp on a)
 *                    L0 = mean_j ( alpha * logp_j - min(Q1, Q2)(obs[i], a_j) )
 *     reg passes:    r  = c(sample(obs[i],         eps_reg[j]).a)                    when any lam != 0
 *                    rn = c(sample(obs_next[i],    eps_next[j]).a)                   when lam_T != 0
 *                    rp = c(sample(obs[i] + noise, eps_pert[j]).a)                   when lam_S != 0;  noise: ONE [obs_dim] row
 *     loss = L0 + lam_T mse(r, rn) + lam_S mse(r, rp) + lam_M mse(r, nominal)        mse: the mean over batch x action_dim elements
 *     alpha_grad = d alpha_loss / d log_alpha = -(target_entropy + mean_j logp_j)    (logp of the loss pass, detached)
 * Four independent noises; the smoothness terms use the regulariser's own sample r, not the loss pass's action.  Gradients flow through
 * both heads in every pass: da/dmean = 1 - a^2, da/dls = (1 - a^2) exp(ls) e, dlogp/du = 2 a (1 - a^2) / (1 - a^2 + 1e-6) and
 * dlogp/dls = -1 beside it; everything through ls is gated by -20 <= raw ls <= 2 (torch.clamp passes the gradient at the bounds), and
 * c(.) by |a| <= max_action.  min(Q1, Q2) sends a row's gradient to the smaller critic, half to each on an exact tie; the critics' own
 * gradients are not produced.  alpha is a constant of this loss.  1 - a^2 and a are formed from t = exp(-2 |u|) as in qr_sac_target,
 * -e^2 / 2 from e.  A coefficient lam_* equal to 0 skips that term's passes and reads none of their inputs; with all three 0 only the
 * loss pass runs.
 *   actor: a QrActor of the QR_ACTOR_TANH_SAMPLE form with the log_std head, in one of the sizes (23,16,4), (15,16,4), (3,4,1).
 *   critic: a QrQCritic whose obs_dim and action_dim equal the actor's; both networks are read.
 *   batch: obs, obs_next (read only with lam_T != 0) and index of a QrTransitions.
 *   eps, eps_reg, eps_next, eps_pert: [batch][action_dim] float32 standard-normal draws, row j for minibatch position j; NULL: zeros
 *   through the same code path.  noise [obs_dim]: required when lam_S != 0; nominal [action_dim]: when lam_M != 0.
 *   alpha: the temperature; alpha_dev, where not NULL, is a device float read in the kernels and wins.  alpha_grad: optional, one float.
 * Outputs, overwritten: the eight gradient tensors in the shapes of the QrActor's, and stats [6] = loss, the mean of min(Q1, Q2), the
 * mean logp of the loss pass, lam_T L_T + lam_S L_S + lam_M L_M, the share of the loss pass's batch x action_dim raw log_std components
 * outside [-20, 2], the share of rows with Q2 < Q1 (both exact counts divided once).
 * Two launches: one wavefront per workgroup accumulates its share of the 64-row tiles and writes ONE partial vector into `workspace`;
 * a second kernel sums the partial vectors in float64 in a fixed order.  The same inputs and grid give the same bits (no atomics).
 * The grid is min(ceil(batch / 64), max_workgroups), max_workgroups = 0: the library's rule (1024). */
typedef struct QrSacActorGrad {
  float *fc1_w, *fc1_b, *fc2_w, *fc2_b, *mean_w, *mean_b, *log_std_w, *log_std_b, *stats;
  const float *eps, *eps_reg, *eps_next, *eps_pert;
  const float* noise;      const float* nominal;
  const float* alpha_dev;  float* alpha_grad;
  void* workspace;         int64_t workspace_bytes;   /* >= qr_sac_actor_workspace_bytes(...); 8-byte aligned */
  float alpha, target_entropy;
  float lam_T, lam_S, lam_M, max_action;
  int32_t max_workgroups, reserved0;
} QrSacActorGrad;
/* QR_E_NULL for a NULL struct, actor weight, critic weight, obs, output or workspace pointer (index, the four eps, alpha_dev and
 * alpha_grad optional; obs_next, noise, nominal as above); QR_E_KIND for squash != QR_ACTOR_TANH_SAMPLE or an actor without the log_std
 * head; QR_E_SIZE for an actor size other than the three above, critic widths outside their ranges, an actor whose obs_dim or
 * action_dim differs from the critic's, reserved0 != 0 (either struct), batch < 1, rows < 1, max_workgroups < 0, a negative or
 * non-finite alpha, max_action or lam_*, a non-finite target_entropy, or a workspace that is too small; QR_E_ALIGN for a float pointer
 * that is not 4-byte aligned or an index / workspace pointer that is not 8-byte aligned.  Nothing is launched or written on an error. */
int qr_sac_actor_grad(const QrActor* actor, const QrQCritic* critic, const QrTransitions* batch, const QrSacActorGrad* grad, void* stream);
/* Bytes of workspace qr_sac_actor_grad needs for this actor size, critic width, batch and max_workgroups; QR_E_SIZE (< 0) where it
 * would refuse them. */
int64_t qr_sac_actor_workspace_bytes(int32_t obs_dim, int32_t hidden_dim, int32_t action_dim, int32_t critic_hidden_dim, int64_t batch,
                                     int32_t max_workgroups);

/* The critic half of one TD3 / SAC minibatch update with ONE centralized twin critic over TWO agents (the reference's CTDE branches:
 * TD3.train, algos/td3/td3.py:124-137, 157-158; SAC.train, algos/sac/sac.py:136-144, 156-157; MLP_Critic_CTDE,
 * algos/td3/td3_mlp.py:102-168), for agent k's reward and done.  The critic is a QrQCritic with obs_dim = obs_dim[0] + obs_dim[1] and
 * action_dim = action_dim[0] + action_dim[1]; its input row is [obs_0 | obs_1 | act_0 | act_1] (torch.cat(state), torch.cat(action)),
 * formed inside the kernels from the two agents' buffers: no concatenated copy of the minibatch exists.
 * What a two-agent ReplayBuffer holds, and one minibatch of it.  Per agent m: obs[m], obs_next[m] [>= rows][obs_dim[m]]; action: row i
 * at action[m] + i * row_stride[m] + col_offset[m]; widths >= 1 each, their sum <= 28.  reward, done: agent k's columns, element i at
 * reward[i * reward_stride], done[i * done_stride].  index, batch, rows: as in QrTransitions.  A pointer the entry point does not read
 * may be NULL: the targets read obs_next, reward, done and index; qr_ctde_twinq_grad reads obs, action and index. */
typedef struct QrCtdeTransitions {
  const float* obs[2];     const float* obs_next[2];
  const float* action[2];
  const float* reward;     const float* done;
  const int64_t* index;
  int64_t batch, rows;
  int32_t obs_dim[2], action_dim[2];
  int32_t row_stride[2], col_offset[2];               /* of the action rows */
  int32_t reward_stride, done_stride;
} QrCtdeTransitions;
/* The TD3 target in ONE launch (td3.py:124-154), j the minibatch position and i = index[j], m = 0, 1:
 *     a'_m = clamp(pi_targ_m(obs_next_m[i]) + clamp(target_noise * eps_m[j], +-noise_clip), +-max_action)
 *     y[j] = reward[i] + discount * (1 - done[i]) * min(Q1_targ, Q2_targ)([obs_next_0[i] | obs_next_1[i] | a'_0 | a'_1])
 * Both actors: QR_ACTOR_TANH_MEAN forms of exactly the sizes (15,16,4) and (3,4,1), the Decoupled wrapper's, equal to the batch's widths.
 * Both actors NULL: a'_m = action_next[m][j] ([batch][action_dim[m]], used as it is), any widths.  One NULL and one not is an error.
 * eps[m]: [batch][action_dim[m]] by minibatch position, or NULL: no noise.  A row with done = 1 gets y = reward exactly. */
typedef struct QrCtdeTd3Target {
  const float* eps[2];
  const float* action_next[2];
  float* y;
  float discount, target_noise, noise_clip, max_action;
} QrCtdeTd3Target;
/* QR_E_NULL for a NULL critic, batch or target struct, weight, obs_next, reward, done or y pointer, exactly one actor NULL, or both
 * NULL with an action_next NULL; QR_E_KIND for an actor with squash != QR_ACTOR_TANH_MEAN or a log_std head; QR_E_SIZE for widths
 * outside the ranges above, widths that do not add up to the critic's, reserved0 != 0, actor sizes other than (15,16,4) and (3,4,1) or
 * different from the batch's widths, batch < 1, rows < 1, a stride < 1 or a negative or non-finite noise_clip / max_action; QR_E_ALIGN
 * for a float pointer that is not 4-byte aligned or an index pointer that is not 8-byte aligned.  Nothing is launched on an error. */
int qr_ctde_twinq_target(const QrActor* actor_target_0, const QrActor* actor_target_1, const QrQCritic* critic_target,
                         const QrCtdeTransitions* batch, const QrCtdeTd3Target* target, void* stream);
/* SAC's soft target in ONE launch (sac.py:136-153), with qr_sac_target's sample and its arithmetic, m = 0, 1 and k = agent:
 *     (mean_m, ls_m) = pi_m(obs_next_m[i]);  ls_m = clamp(ls_m, -20, 2);  a'_m = tanh(mean_m + exp(ls_m) * eps_m[j])     (the LIVE actors)
 *     logp_j = sum_f [ -e^2 / 2 - ls_k - log sqrt(2 pi) - log(1 - tanh(mean_k + exp(ls_k) e)^2 + 1e-6) ],   e = eps_logp[j]
 *     y[j] = reward[i] + discount * (1 - done[i]) * ( min(Q1_targ, Q2_targ)([obs_next_0[i] | obs_next_1[i] | a'_0 | a'_1]) - alpha * logp_j )
 * The reference samples agent k a second time for the log-probability: eps_logp [batch][action_dim[k]] is that draw; NULL: eps[k], one
 * sample, and the same tensor for both gives the bits of NULL.  eps[m] NULL: zeros.  Both actors: QR_ACTOR_TANH_SAMPLE forms with the
 * log_std head, sizes as above.  Both NULL: a'_m = action_next[m][j] and logp_j = logp_next[j] as they are.  alpha, alpha_dev: as in
 * QrSacTarget.  action_out[m] [batch][action_dim[m]] and logp_out [batch]: optional, what was used.  agent: 0 or 1. */
typedef struct QrCtdeSacTarget {
  const float* eps[2];       const float* eps_logp;
  const float* action_next[2];  const float* logp_next;
  const float* alpha_dev;
  float* y;
  float* action_out[2];      float* logp_out;
  float discount, alpha;
  int32_t agent, reserved0;
} QrCtdeSacTarget;
/* As qr_ctde_twinq_target, with: QR_E_NULL also for both actors NULL with logp_next NULL; QR_E_KIND for an actor with squash !=
 * QR_ACTOR_TANH_SAMPLE or without the log_std head; QR_E_SIZE also for agent outside 0..1, reserved0 != 0 (either struct) or a
 * negative or non-finite discount or alpha (no noise_clip / max_action here).  Nothing is launched on an error. */
int qr_ctde_sac_target(const QrActor* actor_0, const QrActor* actor_1, const QrQCritic* critic_target, const QrCtdeTransitions* batch,
                       const QrCtdeSacTarget* target, void* stream);
/* qr_twinq_grad for the centralized critic: the same loss, the same twelve gradients and stats [4], the row x_i = [obs_0[i] | obs_1[i]
 * | act_0[i] | act_1[i]] formed in the kernel's tile from its four sources.  The QrTwinQGrad, the two launches, the grid rule and the
 * workspace are qr_twinq_grad's; with the concatenated rows materialised, qr_twinq_grad gives the same bits at the same grid.
 * QR_E_NULL, QR_E_SIZE and QR_E_ALIGN as qr_twinq_grad, per agent for obs, action, row_stride and col_offset; QR_E_SIZE also for
 * widths < 1 or widths that do not add up to the critic's.  Nothing is launched on an error. */
int qr_ctde_twinq_grad(const QrQCritic* critic, const QrCtdeTransitions* batch, const QrTwinQGrad* grad, void* stream);
/* Bytes of workspace qr_ctde_twinq_grad needs (in_dim = the four widths' sum, >= 4): qr_twinq_workspace_bytes's figure. */
int64_t qr_ctde_twinq_workspace_bytes(int32_t in_dim, int32_t hidden_dim, int64_t batch, int32_t max_workgroups);

/* The actor half of one TD3 minibatch update for agent k of TWO agents under ONE centralized twin critic (the CTDE branch of
 * TD3.train, algos/td3/td3.py:180-196, without the equivariant term, with algos/policy_regularization.py), read from the two agents'
 * buffers in place, without autograd.  With j the minibatch position, i = index[j], c(.) = clamp to +-max_action and m = 0, 1:
 *     a_m     = c(pi_m(obs_m[i]))                             pi = tanh(fc3(relu(fc2(relu(fc1 x)))))     (MLP_Actor_TD3)
 *     loss_k  = -(1/B) sum_j Q1([obs_0[i] | obs_1[i] | a_0 | a_1])
 *               + lam_T mse(a_k, c(pi_k(obs_next_k[i]))) + lam_S mse(a_k, c(pi_k(obs_k[i] + noise))) + lam_M mse(a_k, nominal)
 * and loss_k.backward()'s gradients for agent k's six actor tensors: through all three evaluations of pi_k and through Q1 into a_k
 * alone, dQ/da_k = fc1_w[:, D + off_k .. D + off_k + action_dim[k])^T dz1 with D = obs_dim[0] + obs_dim[1], off_0 = 0 and
 * off_1 = action_dim[0].  The other agent's action enters Q1 as a VALUE only.  (In the reference that agent's actor receives a .grad
 * from this backward pass too; it zeroes it in its own zero_grad() before anything reads it, and neither clip_grad_norm_ nor agent k's
 * optimiser touches it.  Here no gradient for agent 1-k exists and nothing of that actor is written.)
 * noise [obs_dim[k]] (ONE row, broadcast), nominal [action_dim[k]], the coefficients and mse are qr_dpg_actor_grad's: a lam_* equal
 * to 0 skips that term's passes and reads none of its inputs.
 *   agent: k, 0 or 1.  Agent k's actor is a QrActor of the QR_ACTOR_TANH_MEAN form of the Decoupled wrapper's size for that place:
 *   (15,16,4) for agent 0, (3,4,1) for agent 1, equal to the batch's obs_dim[k] and action_dim[k]; its log_std is not read.
 *   The other agent's action, one of two forms:
 *     both actors given, action_other NULL: the pair has exactly the sizes (15,16,4) and (3,4,1) and the batch their widths; pi_{1-k}
 *       runs forward only inside the kernel and its output is clamped.
 *     the actor of agent 1-k NULL, action_other [batch][action_dim[1-k]] float32 by minibatch position: used as it is (no clamp);
 *       the other agent's obs_dim and action_dim are free as long as the four widths add up to the critic's (<= 28).
 *     Both actors AND action_other: QR_E_KIND (the form is ambiguous), reported with the other QR_E_KIND causes, before any size.
 *   critic: a QrQCritic with the summed widths; only fc1 .. fc3 (Q1) are read, fc4 .. fc6 may be NULL.
 *   batch: a QrCtdeTransitions, of which obs[0], obs[1], index and, with lam_T != 0, obs_next[k] are read.
 * Outputs, overwritten: agent k's six gradient tensors and stats [4] = loss_k, the mean of Q1, the share of agent k's B x action_dim[k]
 * components of pi_k(obs_k) with |pi| > max_action (an exact count), and lam_T L_T + lam_S L_S + lam_M L_M.
 * Two launches, the partial vectors, the float64 reduction in a fixed order and the grid rule are qr_dpg_actor_grad's: the same inputs
 * and grid give the same bits (no atomics); grid = min(ceil(batch / 64), max_workgroups), max_workgroups = 0: 1024. */
typedef struct QrCtdeDpgGrad {
  float *fc1_w, *fc1_b, *fc2_w, *fc2_b, *mean_w, *mean_b, *stats;
  const float* noise;      const float* nominal;
  void* workspace;         int64_t workspace_bytes;   /* >= qr_ctde_dpg_actor_workspace_bytes(...); 8-byte aligned */
  float lam_T, lam_S, lam_M, max_action;
  int32_t max_workgroups, reserved0;
  int32_t agent, reserved1;                           /* k; reserved1 must be 0 */
  const float* action_other;
} QrCtdeDpgGrad;
/* In this order: QR_E_NULL for a NULL critic, batch or grad struct; QR_E_KIND for an actor (either) with squash != QR_ACTOR_TANH_MEAN
 * or a log_std head, or both actors together with action_other; QR_E_SIZE for agent outside 0..1, critic widths outside their ranges,
 * widths < 1, widths that do not add up to the critic's or exceed 28, reserved fields != 0, agent k's actor not of its place's size or
 * different from the batch's widths, in the both-actors form a pair other than (15,16,4), (3,4,1), batch < 1, rows < 1,
 * max_workgroups < 0, a negative or non-finite max_action or lam_*; QR_E_NULL for agent k's actor NULL, the other actor and
 * action_other both NULL, a NULL actor weight (agent k's; the other's where it is given), Q1 weight, obs[0], obs[1], output or
 * workspace pointer (index optional; obs_next[k], noise, nominal as above); QR_E_ALIGN for a float pointer that is not 4-byte aligned
 * or an index / workspace pointer that is not 8-byte aligned; QR_E_SIZE for a workspace that is too small.  Nothing is launched on an
 * error. */
int qr_ctde_dpg_actor_grad(const QrActor* actor_0, const QrActor* actor_1, const QrQCritic* critic, const QrCtdeTransitions* batch,
                           const QrCtdeDpgGrad* grad, void* stream);
/* Bytes of workspace qr_ctde_dpg_actor_grad needs for agent 0 (the (15,16,4) actor) or 1 (the (3,4,1) actor), this critic width, batch
 * and max_workgroups: qr_dpg_actor_workspace_bytes' figure for that actor.  QR_E_SIZE (< 0) where the entry would refuse them. */
int64_t qr_ctde_dpg_actor_workspace_bytes(int32_t agent, int32_t critic_hidden_dim, int64_t batch, int32_t max_workgroups);

/* The actor half of one SAC minibatch update for agent k of TWO agents under ONE centralized twin critic (the CTDE branch of
 * SAC.train, algos/sac/sac.py:175-203, without the spectral-norm term, with algos/policy_regularization.py), read from the two agents'
 * buffers in place, without autograd.  sample(.), c(.), the reg passes, mse and the gates are qr_sac_actor_grad's; m = 0, 1:
 *     a_m     = sample(pi_m, obs_m[i], eps_m[j]).a                     (no clamp; eps_k = eps, eps_{1-k} = eps_other)
 *     logp_j  = sample(pi_k, obs_k[i], eps_logp[j]).logp               (a SECOND sample of agent k, sac.py:180)
 *     L0      = mean_j ( alpha * logp_j - min(Q1, Q2)([obs_0[i] | obs_1[i] | a_0 | a_1]) )
 *     loss_k  = L0 + lam_T mse(r, rn) + lam_S mse(r, rp) + lam_M mse(r, nominal)      (r, rn, rp: agent k's, from eps_reg, eps_next, eps_pert)
 *     alpha_grad = -(target_entropy + mean_j logp_j)                   (logp of the SECOND sample)
 * and loss_k.backward()'s gradients for agent k's eight actor tensors.  The Q term reaches pi_k through a_k, the first sample:
 * dQ/da_k = fc1_w[:, D + off_k .. D + off_k + action_dim[k])^T dz1 of the selected critic, D = obs_dim[0] + obs_dim[1], off_0 = 0,
 * off_1 = action_dim[0]; the entropy term through the second sample.  Both samples share one forward pass (the same row gives the same
 * mean and raw log_std) and their deltas add before one backward pass.  eps_logp NULL: ONE sample, drawn with eps — logp and a from
 * the same sample, exactly as qr_sac_actor_grad; eps_logp given as zeros is NOT that form.  The other agent's action enters both critics
 * as a VALUE only.  (In the reference that agent's actor receives a .grad from this backward pass too; it zeroes it in its own
 * zero_grad() before anything reads it.  Here no gradient for agent 1-k exists and nothing of that actor is written.)
 *   QrSacActorGrad's members keep their meaning for agent k (noise [obs_dim[k]], nominal [action_dim[k]], eps = agent k's first draw).
 *   agent: k, 0 or 1.  Agent k's actor is a QrActor of the QR_ACTOR_TANH_SAMPLE form with the log_std head, of the Decoupled wrapper's
 *   size for that place: (15,16,4) for agent 0, (3,4,1) for agent 1, equal to the batch's obs_dim[k] and action_dim[k].
 *   The other agent's action, one of two forms:
 *     both actors given, action_other NULL: the pair has exactly the sizes (15,16,4) and (3,4,1) and the batch their widths; pi_{1-k}
 *       runs forward only inside the kernel, sampled with eps_other [batch][action_dim[1-k]] (NULL: zeros), tanh, no clamp.
 *     the actor of agent 1-k NULL, action_other [batch][action_dim[1-k]] float32 by minibatch position: used as it is; eps_other is
 *       not read; the other agent's obs_dim and action_dim are free as long as the four widths add up to the critic's (<= 28).
 *     Both actors AND action_other: QR_E_KIND (the form is ambiguous), reported with the other QR_E_KIND causes, before any size.
 *   critic: a QrQCritic with the summed widths; both networks are read.
 *   batch: a QrCtdeTransitions, of which obs[0], obs[1], index and, with lam_T != 0, obs_next[k] are read.
 * Outputs, overwritten: agent k's eight gradient tensors, stats [6] as qr_sac_actor_grad's (stats[2] = the mean logp that enters the
 * loss: the second sample's where eps_logp is given; stats[4] counts agent k's raw log_std) and, where not NULL, alpha_grad.
 * Two launches, the partial vectors (qr_sac_actor_grad's for agent k's actor size), the float64 reduction in a fixed order and the grid
 * rule are qr_sac_actor_grad's: the same inputs and grid give the same bits (no atomics). */
typedef struct QrCtdeSacActorGrad {
  float *fc1_w, *fc1_b, *fc2_w, *fc2_b, *mean_w, *mean_b, *log_std_w, *log_std_b, *stats;
  const float *eps, *eps_reg, *eps_next, *eps_pert;
  const float* noise;      const float* nominal;
  const float* alpha_dev;  float* alpha_grad;
  void* workspace;         int64_t workspace_bytes;   /* >= qr_ctde_sac_actor_workspace_bytes(...); 8-byte aligned */
  float alpha, target_entropy;
  float lam_T, lam_S, lam_M, max_action;
  int32_t max_workgroups, reserved0;
  int32_t agent, reserved1;                           /* k; reserved1 must be 0 */
  const float* eps_logp;
  const float* eps_other;
  const float* action_other;
} QrCtdeSacActorGrad;
/* In this order: QR_E_NULL for a NULL critic, batch or grad struct; QR_E_KIND for an actor (either) with squash !=
 * QR_ACTOR_TANH_SAMPLE or without the log_std head, or both actors together with action_other; QR_E_SIZE for agent outside 0..1, critic
 * widths outside their ranges, widths < 1, widths that do not add up to the critic's or exceed 28, reserved fields != 0, agent k's
 * actor not of its place's size or different from the batch's widths, in the both-actors form a pair other than (15,16,4), (3,4,1),
 * batch < 1, rows < 1, max_workgroups < 0, a negative or non-finite alpha, max_action or lam_*, a non-finite target_entropy; QR_E_NULL
 * for agent k's actor NULL, the other actor and action_other both NULL, a NULL actor weight (agent k's; the other's where it is given),
 * critic weight, obs[0], obs[1], output or workspace pointer (index, the draws, alpha_dev and alpha_grad optional; obs_next[k], noise,
 * nominal as in qr_sac_actor_grad); QR_E_ALIGN for a float pointer that is not 4-byte aligned or an index / workspace pointer that is
 * not 8-byte aligned; QR_E_SIZE for a workspace that is too small.  Nothing is launched or written on an error. */
int qr_ctde_sac_actor_grad(const QrActor* actor_0, const QrActor* actor_1, const QrQCritic* critic, const QrCtdeTransitions* batch,
                           const QrCtdeSacActorGrad* grad, void* stream);
/* Bytes of workspace qr_ctde_sac_actor_grad needs for agent 0 (the (15,16,4) actor) or 1 (the (3,4,1) actor), this critic width, batch
 * and max_workgroups: qr_sac_actor_workspace_bytes' figure for that actor.  QR_E_SIZE (< 0) where the entry would refuse them. */
int64_t qr_ctde_sac_actor_workspace_bytes(int32_t agent, int32_t critic_hidden_dim, int64_t batch, int32_t max_workgroups);

/* ---- The replay buffer of TD3 / SAC: append and minibatch indices (algos/replay_buffer.py) ----
 * The buffer is, per agent k, five flat device tensors of `capacity` rows: obs, obs_next [capacity][obs_dim[k]], action
 * [capacity][action_dim[k]], reward, done [capacity] float32 (done: 0.0 / 1.0) — what QrTransitions / QrCtdeTransitions read.  Three
 * counters go with it: count (the next row to write), current_size (the rows that hold a transition) and draw (the minibatches drawn).
 * They live on the host and are passed by value, or — `state` not NULL — in device memory as int64 state[3] = {count, current_size,
 * draw}: then both entries read them there and advance them there, with a one-thread launch of its own on the same stream behind the
 * launch that read them, so a stream (or a captured graph of it) can append and sample any number of times without the host.
 *
 * The append of one collected horizon of n_steps x n_envs transitions in ONE launch (plus the counters' where state is given), for one or
 * two agents.  Transition j = t * n_envs + n goes to ring row (count + j) mod capacity:
 *     buf_obs[k][row]      = obs[k][t][n]
 *     buf_obs_next[k][row] = final_obs[k][t][n]  where final_obs is given and any agent's done[t][n][.] or truncated[t][n] is set
 *                          = obs[k][t + 1][n]    elsewhere
 *     buf_action[k][row]   = action[t][n][col_offset[k] .. col_offset[k] + action_dim[k])
 *     buf_reward[k][row]   = reward[t][n][k]        buf_done[k][row] = done[t][n][k] ? 1.0 : 0.0
 * Values are copied bit for bit; no temporaries are made; rows outside the n_steps * n_envs written ones are not touched.  count is not
 * advanced on the host's behalf: the caller's next count is (count + n_steps * n_envs) mod capacity, its current_size
 * min(current_size + n_steps * n_envs, capacity) — which is what the device counters become. */
typedef struct QrReplayAdd {
  const float* obs[2];            /* [n_steps + 1][n_envs][obs_dim[k]] */
  const float* final_obs[2];      /* [n_steps][n_envs][obs_dim[k]]; all NULL: obs_next is obs[t + 1] everywhere */
  const float* action;            /* [n_steps][n_envs][action_row]: the agents' actions side by side */
  const float* reward;            /* [n_steps][n_envs][n_agents] */
  const uint8_t* done;            /* [n_steps][n_envs][n_agents] bool bytes */
  const uint8_t* truncated;       /* [n_steps][n_envs] bool bytes, or NULL */
  float* buf_obs[2];      float* buf_obs_next[2];   float* buf_action[2];   float* buf_reward[2];   float* buf_done[2];
  int64_t* state;                 /* NULL, or device int64[3] = {count, current_size, draw}: read instead of `count`, then advanced */
  int64_t count;                  /* the next row to write, 0 <= count < capacity (state NULL) */
  int64_t capacity, n_envs;
  int32_t n_steps, n_agents;      /* n_agents 1 or 2 */
  int32_t obs_dim[2], action_dim[2], col_offset[2];   /* 1 .. 4096 each width; col_offset[k] + action_dim[k] <= action_row */
  int32_t action_row, reserved0;  /* reserved0 must be 0 */
} QrReplayAdd;
/* In this order: QR_E_NULL for a NULL struct; QR_E_SIZE for n_agents outside 1..2, reserved0 != 0, capacity < 1, n_steps < 1, n_envs < 1,
 * n_steps * n_envs > capacity, count outside [0, capacity) where state is NULL, a width outside 1..4096, a column range outside the
 * action row; QR_E_NULL for a NULL obs, action, reward, done or buffer pointer of an agent in use, or final_obs given for one agent only;
 * QR_E_ALIGN for a float pointer that is not 4-byte aligned or a state pointer that is not 8-byte aligned.  Nothing is launched or
 * written on an error.  Members of agent 1 are not read when n_agents is 1. */
int qr_replay_add(const QrReplayAdd* add, void* stream);

/* The same append with the reference's time-limit "solved" rule in the done it stores (main.py:169-173): at the episode time limit the
 * reference overwrites done_n with "the error is within tolerance and the agent did not crash".  For transition (t, n) and agent k:
 *     limit           = truncated[t][n] != 0
 *     src_k           = the row buf_obs_next[k] receives for (t, n): final_obs[k][t][n] where final_obs is given (truncated is set, so
 *                       the env was re-sampled), obs[k][t + 1][n] otherwise
 *     solved_0        = fabs((double)src_0[c] * x_lim) <= pos_tol for c = 0, 1, 2     (ex, de-normalised: utils/utils.py:21-39)
 *     solved_1        = fabs((double)src_1[0] * pi) <= rot_tol                        (eb1; pi = the double nearest pi; two agents only)
 *     buf_done[k][row] = limit ? (solved_k && reward[t][n][k] != -1.0f ? 1.0 : 0.0) : (done[t][n][k] ? 1.0 : 0.0)
 * One agent (Coupled) is agent 0 alone and its rule reads ex alone, as the reference's MONO branch does.  The comparisons are made in
 * double on the float32 words.  -1.0f is the crash reward as the step kernels store it (a literal, not arithmetic).  Everything else —
 * the other four tensors, the ring rows, the wrap, the device counters — is qr_replay_add's, bit for bit, in the same single launch. */
typedef struct QrReplayAddRule {
  QrReplayAdd add;                /* truncated and reward are required here */
  double x_lim;                   /* the env's position limit (QrCoeffs.x_lim), > 0 */
  double pos_tol, rot_tol;        /* [m], [rad]; the reference's are 0.03 and 0.03; finite, >= 0 */
} QrReplayAddRule;
/* qr_replay_add's errors in qr_replay_add's order, with: QR_E_SIZE also for a non-finite or negative pos_tol or rot_tol, an x_lim that is
 * not finite and > 0, or obs_dim[0] < 3; QR_E_NULL also for a NULL truncated.  Nothing is launched or written on an error. */
int qr_replay_add_rule(const QrReplayAddRule* rule, void* stream);

/* `batch` pairwise distinct rows below n, in O(batch) and in integers only: index[j] is the image of j under a keyed pseudo-random
 * permutation of [0, n), so the same (n, seed, draw) gives the same indices on any device, launch geometry or CPU restatement.
 *     h    = max(1, ceil(bit_length(n - 1) / 2)),  mask = 2^h - 1
 *     P(x) : (L, R) = (x >> h, x & mask); six times, r = 0..5: (L, R) <- (R, L xor (F & mask)), F = word 0 of Philox4x32-10 with the
 *            counter (R, r, draw_lo, draw_hi) under the key (seed_lo, seed_hi); P(x) = L << h | R  — a permutation of [0, 4^h)
 *     index[j] = the first of P(j), P(P(j)), ... that is below n  (cycle walking: a permutation of [0, n))
 * The walk starts below n and follows a cycle of P, which has 4^h < 4 n points, so it ends; it is capped at 4^h steps all the same, and a
 * capped walk stores 0 and sets *status to 1 (status may be NULL; it is never cleared here).  A (seed, draw) pair must not be used
 * twice: draw counts the calls.  With state, n = state[1] and draw = state[2] are read on the device (the members n and draw are
 * then only checked), and state[2] is advanced by one behind the launch. */
typedef struct QrReplaySample {
  int64_t* index;                 /* [batch], written */
  int32_t* status;                /* NULL or one device word */
  int64_t* state;                 /* NULL, or device int64[3] = {count, current_size, draw} */
  int64_t n, batch;               /* 1 <= batch <= n < 2^31 */
  uint64_t seed, draw;
} QrReplaySample;
/* QR_E_NULL for a NULL struct; QR_E_SIZE for batch < 1, batch > n or n >= 2^31; QR_E_NULL for a NULL index; QR_E_ALIGN for an index or
 * state pointer that is not 8-byte aligned or a status pointer that is not 4-byte aligned.  Nothing is launched or written on an error. */
int qr_replay_sample(const QrReplaySample* sample, void* stream);

/* ---- The library's noise source: every random tensor of a TD3 / SAC iteration in one launch ----
 * Up to sixteen float32 tensors ("slots") filled from one counter-based stream, keyed by a 64-bit seed, a draw number — the replay
 * buffer's minibatch counter, so that an iteration's noise is a function of its minibatch number — and a stream id per slot.
 * Element e of a slot is position e % 4 of quad q = e / 4.  The quad's four 32-bit words are Philox4x32-10 under the key
 * (seed_lo, seed_hi) with the counter
 *     { (uint32)q, (uint32)(q >> 32) ^ (uint32)(draw >> 32), (uint32)draw, 0x80000000 | 0x40000000 | stream }
 * (the rollout noise's counter layout with bit 30 set in its last word, which no other stream of the library sets together with
 * the top bit).  QR_NOISE_NORMAL: words (0, 1) and (2, 3) each give a Box-Muller pair, in float32: u = fma(w >> 8, 2^-24, 2^-25),
 * r = sqrt(-2 log u1), z = (r cos(2 pi u2), r sin(2 pi u2)) — the rollout noise's arithmetic; out[e] = fma(b, z, a), so a is the
 * mean and b the standard deviation.  QR_NOISE_UNIFORM: s = fma(w >> 8, 2^-23, 2^-24 - 1), uniform on a grid of 2^24 points in
 * (-1, 1); out[e] = fma(b, s, a).  A value depends on (seed, draw, stream, e, kind, a, b) alone: not on the slot's position, the
 * other slots, the launch geometry or the pointer's alignment.  A (seed, draw, stream) triple must not be used for two tensors.
 * draw_dev: NULL, or one device int64 that the launch READS as the draw number (it is never written), for callers whose counter
 * lives on the device (QrReplaySample.state + 2); `draw` is then ignored. */
#define QR_NOISE_MAX_SLOTS 16
#define QR_NOISE_NORMAL  0   /* out[e] = fmaf(b, z, a), z standard normal: a = mean, b = std        */
#define QR_NOISE_UNIFORM 1   /* out[e] = fmaf(b, s, a), s uniform in (-1, 1)                         */
typedef struct QrNoiseSlot {
  float* out;                     /* [count], written; 4-byte aligned (16-byte aligned: 16-byte stores) */
  int64_t count;                  /* >= 1; the launch's quads, the sum of ceil(count / 4) over its slots, stay below 2^31 */
  float a, b;
  uint32_t kind, stream;          /* QR_NOISE_*; stream < 2^30 */
} QrNoiseSlot;
typedef struct QrNoiseFill {
  QrNoiseSlot slot[QR_NOISE_MAX_SLOTS];
  int32_t n_slots;                /* 1..16 */
  uint64_t seed;
  const int64_t* draw_dev;        /* NULL, or one device int64 that is READ as the draw number (never written) */
  int64_t draw;                   /* the draw number where draw_dev is NULL: >= 0 */
} QrNoiseFill;
/* QR_E_NULL for a NULL struct; QR_E_SIZE for n_slots outside 1..16, a count < 1 or more than 2^31 - 1 quads in the launch, a kind outside {0, 1}, a stream >= 2^30,
 * a non-finite a or b, or a negative draw where draw_dev is NULL; QR_E_NULL for a NULL out; QR_E_ALIGN for an out that is not 4-byte
 * aligned or a draw_dev that is not 8-byte aligned.  One launch.  Nothing is launched or written on an error. */
int qr_noise_fill(const QrNoiseFill* fill, void* stream);

/* ---- Per-episode training statistics from a collected horizon (the reference's training curve, main.py:132-137, 180, 212-235) ----
 * A scan over the [n_steps][n_envs] rows a horizon has already written (qr_rollout / qr_rollout_actor with QR_FLAG_AUTO_RESET): one lane
 * per env walks t = 0 .. n_steps - 1 with two carries per env that live on the device across calls,
 *     run_return[n][g] += (double)reward[t][n][g]        run_length[n] += 1           (the terminal step counts)
 * and the episode of env n ENDS in step t when any agent's done[t][n][.] or truncated[t][n] is set (the rule of qr_replay_add's obs_next
 * and of qr_critic_next_values).  At an end the lane forms the episode's record and clears the env's carries:
 *     return[g]  = run_return[n][g]: float64, the sum of the float32 rewards, NOT rounded.  Deliberate deviation, the one
 *                  QrEvalOut.episode_return documents: the reference rounds its running sum to 4 decimals at every step (main.py:180).
 *     length     = run_length[n]
 *     flags      = QR_EP_FLAG_DONE0 << g where agent g's done is set | QR_EP_FLAG_TRUNCATED where truncated is set
 *                | QR_EP_FLAG_SOLVED0 << g where truncated is set and agent g is "solved" (main.py:169-173, qr_replay_add_rule's rule):
 *                  agent 0: fabs(ex[c]) <= pos_tol for c = 0, 1, 2 and reward[t][n][0] != -1.0f; agent 1: fabs(eb1) <= rot_tol and
 *                  reward[t][n][1] != -1.0f
 *     ex[c]      = (double)final_obs0[t][n][c] * x_lim,  eb1 = (double)final_obs1[t][n][0] * pi (pi the double nearest pi; 0 with one
 *                  agent): qr_replay_add_rule's expressions, compared in double on the float32 words; stored as (float)
 * final_obs0 NULL: ex, eb1 and the solved bits are zero (final_obs1 is then not read), and ep_final_error must be NULL.
 * Dense per-transition outputs, each may be NULL; a row where no episode ended holds zeros, so ep_length > 0 is the mask of the ends and
 * its non-zeros in (t, n) order are the reference's log lines in the reference's order:
 *     ep_return [n_steps][n_envs][n_agents] float64   ep_length [n_steps][n_envs] int32   ep_flags [n_steps][n_envs] uint8
 *     ep_final_error [n_steps][n_envs][4] float32: ex (3), eb1
 * Statistics over the episodes that ended in this launch: QR_EP_FIELDS float64 fields, agent g's at index + g (one agent: agent 1's
 * fields stay empty).  An empty field is +inf for a minimum, -inf for a return's maximum, 0 elsewhere. */
#define QR_EP_COUNT        0   /* episodes */
#define QR_EP_RETURN_SUM   1   /* +g: sum of returns */
#define QR_EP_RETURN_SQ    3   /* +g: sum of squared returns */
#define QR_EP_RETURN_MIN   5   /* +g */
#define QR_EP_RETURN_MAX   7   /* +g */
#define QR_EP_LENGTH_SUM   9
#define QR_EP_LENGTH_MAX  10
#define QR_EP_DONE        11   /* +g: episodes whose last step has agent g's done set */
#define QR_EP_TRUNCATED   13   /* episodes whose last step has truncated set */
#define QR_EP_SOLVED      14   /* +g: episodes with agent g's solved bit */
#define QR_EP_EX_SUM      16   /* sum of max_c |ex[c]| (double) */
#define QR_EP_EB1_SUM     17   /* sum of |eb1| (double) */
#define QR_EP_FIELDS      18   /* K: the length of `last` and of a workgroup's partial vector */
#define QR_EP_STEPS_SEEN  18   /* `total` only: env-steps per env scanned so far; advances by n_steps with every call */
#define QR_EP_TOTAL_FIELDS 19  /* the length of `total` */
#define QR_EP_FLAG_DONE0      0x01u   /* << g */
#define QR_EP_FLAG_SOLVED0    0x10u   /* << g */
#define QR_EP_FLAG_TRUNCATED  0x80u
/* Each 64-env workgroup reduces its lanes' fields with a fixed shuffle tree into one vector of `workspace`; a second launch of one
 * workgroup folds the vectors in workgroup-index order (256 strided slices, then a tree) — no floating-point atomics, and a result that
 * does not depend on which workgroup finished first — into
 *     last[QR_EP_FIELDS]         this call's statistics
 *     total[QR_EP_TOTAL_FIELDS]  since the caller zeroed it (an empty vector: the fields' empty values, steps_seen 0): sums and counts
 *                                add, minima and maxima fold.  Both are additive / foldable over env shards in the same way.
 * record = 0 (main.py:218: episodes that end during the warm-up are not logged): the carries advance and are cleared as ever and the
 * dense rows are written, `last` is an empty vector and `total` keeps every field but steps_seen. */
typedef struct QrEpisodeScan {
  const float*   reward;          /* [n_steps][n_envs][n_agents]; two agents: 8-byte aligned */
  const uint8_t* done;            /* [n_steps][n_envs][n_agents] bool bytes */
  const uint8_t* truncated;       /* [n_steps][n_envs] bool bytes */
  const float*   final_obs0;      /* [n_steps][n_envs][d0] or NULL; read on the rows where an episode ended only */
  const float*   final_obs1;      /* [n_steps][n_envs][d1]; required with two agents where final_obs0 is given */
  double*        run_return;      /* [n_envs][n_agents], read and written */
  int32_t*       run_length;      /* [n_envs], read and written */
  double*        ep_return;       /* the four dense outputs, each may be NULL */
  int32_t*       ep_length;
  uint8_t*       ep_flags;
  float*         ep_final_error;  /* 16-byte aligned */
  double*        last;            /* [QR_EP_FIELDS], written */
  double*        total;           /* [QR_EP_TOTAL_FIELDS], read and written */
  void*          workspace;       int64_t workspace_bytes;   /* >= qr_episode_workspace_bytes(n_envs); 8-byte aligned */
  int64_t        n_envs;
  int32_t        n_steps, n_agents;   /* n_agents 1 or 2 */
  int32_t        d0, d1;          /* row widths of final_obs0 / final_obs1: d0 >= 3, d1 >= 1 (two agents) */
  int32_t        record, reserved0;   /* reserved0 must be 0 */
  double         x_lim;           /* the env's position limit (QrCoeffs.x_lim), finite and > 0 */
  double         pos_tol, rot_tol;/* [m], [rad]; the reference's are 0.03 and 0.03; finite, >= 0 */
} QrEpisodeScan;
/* Two launches on `stream` behind one call; no host synchronisation, no allocation.  In this order, all before any launch: QR_E_NULL for
 * a NULL struct; QR_E_SIZE for n_steps < 1, n_envs < 0 or > 2^36, n_agents outside 1..2, reserved0 != 0, d0 < 3, d1 < 1 with two agents, an x_lim
 * that is not finite and > 0, a negative or non-finite tolerance or a workspace that is too small; QR_E_NULL for a NULL reward, done,
 * truncated, run_return, run_length, last, total or workspace, a NULL final_obs1 with two agents where final_obs0 is given, or an
 * ep_final_error where final_obs0 is NULL; QR_E_ALIGN for a float or int32 pointer that is not 4-byte aligned, a double or workspace
 * pointer that is not 8-byte aligned, a two-agent reward that is not 8-byte aligned or an ep_final_error that is not 16-byte aligned.
 * n_envs = 0 launches nothing. */
int     qr_episode_scan(const QrEpisodeScan* a, void* stream);
/* Bytes of workspace qr_episode_scan needs: one vector of QR_EP_FIELDS doubles per 64-env workgroup (at least one); QR_E_SIZE (< 0)
 * for n_envs < 0. */
int64_t qr_episode_workspace_bytes(int64_t n_envs);

/* ---- PPO's advantages with the done flag the reference stores, their statistics and their normalisation in one call ----
 * main.py:169-173 overwrites done_n at the episode time limit with "solved and not crashed", main.py:176-177 stores that flag for PPO,
 * and ppo.py:134-146 reads it twice: in td_error = r + gamma * V(obs_next) * (1 - done) - V and in the (1 - done) that cuts the
 * lambda-recursion.  qr_gae_rule is qr_gae's reverse scan over the EFFECTIVE flag of transition (t, n) and agent k:
 *     done_eff = done[t][n][k]                                             where truncated[t][n] == 0, or rule == 0
 *              = solved_k && reward[t][n][k] != -1.0f                      where truncated[t][n] != 0 and rule == 1
 *     solved_0 = fabs((double)term_obs0[t][n][c] * x_lim) <= pos_tol for c = 0, 1, 2
 *     solved_1 = fabs((double)term_obs1[t][n][0] * pi) <= rot_tol          (pi = the double nearest pi; two agents only)
 * — qr_replay_add_rule's expressions, compared in double on the float32 words; an own done = 1 on a time-limit row is overridden.
 * term_obs0 / term_obs1 hold the transition's obs_next on time-limit rows: final_obs where the storage has it, else the rows
 * obs[k][1:] (qr_replay_add_rule's choice); they are read on rows whose truncated is set only (three words, one word).
 *     nd = done_eff ? 0 : 1;  delta = r + gamma * Vnext * nd - V;  adv = delta + gamma * nd * lam * adv;  td_target = adv + V
 * in float32, qr_gae's recurrence expression for expression: advantage and td_target equal qr_gae run on done_eff bit for bit.
 * value / next_value mean what they mean for qr_gae: without next_value, row n_steps of value is the bootstrap.
 * Bootstrap semantics are otherwise unchanged (qr_critic_next_values supplies V(final_obs) on reset rows); the reference's
 * cross-episode leak on unsolved time limits is kept.
 * stats: per agent the sum and the sum of squares of its advantages in float64 and the count n_steps * n_envs as a double — the layout
 * RolloutStorage.normalize consumes.  Each lane accumulates in float64, a fixed shuffle tree over the lanes of one agent gives one
 * vector per 64-column workgroup in `workspace`, a second launch folds the vectors in workgroup-index order: no floating-point atomics,
 * the same bits from call to call.
 * normalized = (float)(((double)adv - mean) / (std + norm_eps)), mean = s1 / n, var = max(0, (s2 - n * mean * mean) / (n - 1)),
 * std = sqrt(var): ppo.py:146 with torch's unbiased std, per agent, in a third launch that reads stats from device memory. */
typedef struct QrGaeRule {
  const float*   reward;          /* [n_steps][n_envs][n_agents] */
  const uint8_t* done;            /* [n_steps][n_envs][n_agents] bool bytes */
  const uint8_t* truncated;       /* [n_steps][n_envs] bool bytes; required where rule != 0 */
  const float*   term_obs0;       /* [n_steps][n_envs][d0]; required where rule != 0 */
  const float*   term_obs1;       /* [n_steps][n_envs][d1]; required where rule != 0 with two agents */
  const float*   value;           /* [n_steps + 1][n_envs][n_agents] ([n_steps] rows are read where next_value is given) */
  const float*   next_value;      /* [n_steps][n_envs][n_agents], or NULL */
  float*         advantage;       /* [n_steps][n_envs][n_agents], written */
  float*         td_target;       /* [n_steps][n_envs][n_agents], written */
  uint8_t*       done_eff;        /* [n_steps][n_envs][n_agents], written: the done_n the reference would have stored; may be NULL */
  double*        stats;           /* [n_agents][3] = sum, sum of squares, count; may be NULL */
  float*         normalized;      /* [n_steps][n_envs][n_agents]; may be NULL; needs stats and n_steps * n_envs >= 2 */
  void*          workspace;       int64_t workspace_bytes;   /* with stats: >= qr_gae_rule_workspace_bytes(n_envs, n_agents); 8-byte aligned */
  int64_t        n_envs;
  int32_t        n_steps, n_agents;   /* n_agents 1 or 2 */
  int32_t        d0, d1;          /* row widths of term_obs0 / term_obs1; rule != 0: d0 >= 3, d1 >= 1 (two agents) */
  int32_t        rule, reserved0; /* rule 0 or 1; reserved0 must be 0 */
  float          gamma, lam;
  double         x_lim;           /* rule != 0: the env's position limit, finite and > 0 */
  double         pos_tol, rot_tol;/* rule != 0: [m], [rad]; the reference's are 0.03 and 0.03; finite, >= 0 */
  double         norm_eps;        /* the reference's is 1e-4; finite, >= 0 (read with normalized only) */
} QrGaeRule;
/* Up to three launches on `stream` behind one call; no host synchronisation, no allocation.  In this order, all before any launch:
 * QR_E_NULL for a NULL struct; QR_E_SIZE for n_steps < 1, n_envs < 0 or > 2^35, n_agents outside 1..2, reserved0 != 0, rule outside
 * 0..1, with rule != 0 d0 < 3, d1 < 1 with two agents, an x_lim that is not finite and > 0 or a negative or non-finite tolerance, with
 * normalized a negative or non-finite norm_eps or n_steps * n_envs < 2, with stats a workspace that is too small; QR_E_NULL for a NULL
 * reward, done, value, advantage or td_target, with rule != 0 a NULL truncated, term_obs0 or (two agents) term_obs1, normalized without
 * stats, stats without workspace; QR_E_ALIGN for a float pointer that is not 4-byte aligned or a stats or workspace pointer that is
 * not 8-byte aligned.  n_envs = 0 launches nothing. */
int     qr_gae_rule(const QrGaeRule* a, void* stream);
/* Bytes of workspace qr_gae_rule needs with stats: 2 * n_agents doubles per 64-column workgroup (at least one); QR_E_SIZE (< 0) for
 * n_envs < 0 or n_agents outside 1..2. */
int64_t qr_gae_rule_workspace_bytes(int64_t n_envs, int32_t n_agents);

/* ---- An evolution-strategy generation around qr_evaluate_population: the perturbed population and the gradient estimator ----
 * The base theta is a list of up to sixteen float32 tensors (an actor's weights and biases).  Tensor i has count_i elements,
 * Q_i = ceil(count_i / 4) quads and a stream id s_i < 2^30.  The population has P policies, P even, in antithetic adjacent pairs.
 * THE PERTURBATION STREAM: eps_j[e], the draw of pair j (0 <= j < P / 2) for element e of tensor i, is element j * 4 Q_i + e of the
 * qr_noise_fill stream (seed, draw = generation, stream = s_i, QR_NOISE_NORMAL, a = 0, b = 1): quad j * Q_i + e / 4, position e % 4.
 * So the eps of a generation is, bit for bit, what qr_noise_fill writes into a [P / 2][4 Q_i] tensor under that key; it is never
 * stored: both entries regenerate it, and a generation is a function of (seed, generation) alone.  A (seed, generation, stream)
 * triple must not be used for two tensors.  generation_dev: NULL, or one device int64 that the launches READ as the generation (it is
 * never written); `generation` is then ignored.
 *
 * qr_es_perturb, one launch:  d = fl32(sigma * eps_j[e]);  out[2j][e] = fl32(base[e] + d);  out[2j + 1][e] = fl32(base[e] - d)
 * — two roundings each, the product never fused into the sum.  copy[c]: a tensor that is not perturbed (the log_std source) is
 * written to all P rows of its stacked tensor in the same launch.  A value does not depend on the tensor's place in the launch, the
 * other tensors, max_workgroups or a pointer's alignment (16-byte aligned rows get 16-byte stores). */
#define QR_ES_MAX_TENSORS  16
#define QR_ES_MAX_COPIES   8
#define QR_ES_MAX_POLICIES 8192
typedef struct QrEsTensor {
  const float* base;              /* [count]; qr_es_perturb only */
  float*       out;               /* qr_es_perturb: the stacked tensor [P][count], written; qr_es_gradient: grad [count], written */
  int64_t      count;             /* 1 .. 2^31 - 1; (P / 2) * the sum of ceil(count / 4) over the tensors stays below 2^31 */
  uint32_t     stream, reserved0; /* stream < 2^30, pairwise distinct; reserved0 must be 0 */
} QrEsTensor;
typedef struct QrEsCopy {
  const float* src;               /* [count] */
  float*       dst;               /* [P][count], written */
  int64_t      count;             /* 1 .. 2^31 - 1 */
} QrEsCopy;
typedef struct QrEsPerturb {
  QrEsTensor tensor[QR_ES_MAX_TENSORS];
  QrEsCopy   copy[QR_ES_MAX_COPIES];
  int32_t    n_tensors, n_copies; /* 1..16, 0..8 */
  int32_t    n_policies;          /* P: even, 2 .. QR_ES_MAX_POLICIES */
  int32_t    max_workgroups;      /* 0: the library's choice; > 0: a cap on the grid (it cannot change a value) */
  float      sigma, reserved0;    /* sigma finite and > 0; reserved0 must be 0 */
  uint64_t   seed;
  const int64_t* generation_dev;  /* NULL, or one device int64 that is READ as the generation (never written) */
  int64_t    generation;          /* the generation where generation_dev is NULL: >= 0 */
} QrEsPerturb;
/* In this order, all before the launch: QR_E_NULL for a NULL struct; QR_E_SIZE for an odd P, P < 2 or > 8192, n_tensors outside 1..16,
 * n_copies outside 0..8, a count < 1 or too many quads, a stream >= 2^30 or one that appears twice, a reserved0 != 0, a sigma that is
 * not finite and > 0, max_workgroups < 0 or a negative generation where generation_dev is NULL; QR_E_NULL for a NULL base, out, src or
 * dst; QR_E_ALIGN for a float pointer that is not 4-byte aligned or a generation_dev that is not 8-byte aligned.  Nothing is launched
 * or written on an error. */
int qr_es_perturb(const QrEsPerturb* p, void* stream);

/* qr_es_gradient, two launches behind one call.
 * Utilities: fitness [P] float32 -> w [P / 2] float64 in the workspace, w_j = u_2j - u_2j+1.
 *   QR_ES_CENTERED_RANK  rank_i = #{k : f_k < f_i} + 0.5 * (#{k : f_k == f_i} - 1),  u_i = rank_i / (P - 1) - 0.5.  A NaN is ranked as
 *                        -inf is (NaNs tie with each other and with -inf).  The counts are integers: u_i is exact up to its one
 *                        division and one subtraction in float64, and equal fitness everywhere gives every w_j = 0 exactly.
 *   QR_ES_STANDARDIZE    u_i = (f_i - mean) / (std + 1e-8), mean and the unbiased std in float64 in index order; w_j is formed as
 *                        ((double)f_2j - (double)f_2j+1) / (std + 1e-8), in which the mean has cancelled.  With a non-finite fitness
 *                        every w_j = 0.
 * stats [QR_ES_STATS] float64: the fitness mean (float64, index order), the largest fitness and the index of its first occurrence
 * (NaNs are passed over; -inf and 0 where no value compares larger), and 1.0 where a fitness is NaN or infinite, else 0.0.
 * Estimator: for every element of every tensor
 *     grad[e] = fl32( -( sum_j w_j * (double)eps_j[e] ) / (P * sigma) )
 * with eps regenerated from the key.  The sum is float64 in one fixed order — the 64 lanes of a wave stride over j, then a fixed
 * shuffle tree — and rounded to float32 once: no floating-point atomics, the same bits from call to call and for any max_workgroups.
 * The sign makes it a DESCENT gradient of -fitness: an optimiser step on it ascends the fitness. */
#define QR_ES_CENTERED_RANK 0
#define QR_ES_STANDARDIZE   1
#define QR_ES_STATS         4   /* mean, max, argmax, non-finite flag */
typedef struct QrEsGradient {
  QrEsTensor tensor[QR_ES_MAX_TENSORS];   /* out = grad [count]; base is not read */
  const float* fitness;           /* [P] */
  double*    stats;               /* [QR_ES_STATS], written; 8-byte aligned */
  void*      workspace;           int64_t workspace_bytes;   /* >= qr_es_workspace_bytes(P); 8-byte aligned */
  int32_t    n_tensors;           /* 1..16 */
  int32_t    n_policies;          /* P: even, 2 .. QR_ES_MAX_POLICIES */
  int32_t    shaping;             /* QR_ES_CENTERED_RANK or QR_ES_STANDARDIZE */
  int32_t    max_workgroups;      /* 0: the library's choice; > 0: a cap on the estimator's grid (it cannot change a value) */
  float      sigma, reserved0;    /* sigma finite and > 0; reserved0 must be 0 */
  uint64_t   seed;
  const int64_t* generation_dev;
  int64_t    generation;
} QrEsGradient;
/* In this order, all before any launch: QR_E_NULL for a NULL struct; QR_E_SIZE for what qr_es_perturb refuses in its sizes, a shaping
 * outside 0..1 or a workspace that is too small; QR_E_NULL for a NULL grad, fitness, stats or workspace; QR_E_ALIGN for a float
 * pointer that is not 4-byte aligned or a stats, workspace or generation_dev pointer that is not 8-byte aligned.  No host
 * synchronisation, no allocation.  Nothing is launched or written on an error. */
int     qr_es_gradient(const QrEsGradient* g, void* stream);
/* Bytes of workspace qr_es_gradient needs: P / 2 doubles; QR_E_SIZE (< 0) for an odd P, P < 2 or P > 8192. */
int64_t qr_es_workspace_bytes(int32_t n_policies);

/* ---- A keyed permutation of [0, n): PPO's epoch shuffle (ppo.py:158) with no sort, no state and no stored table ----
 *     out[i] = perm(first + i)   for i < count, as int64
 * perm is a bijection of [0, n) and a function of (seed, draw, stream, n) ALONE: not of the grid, of first / count (a slice holds the
 * same values as those positions of the whole, so a rank can form just its own rows), of other calls or of torch's generator.
 *   n = 1: perm = {0}.  Otherwise w = the smallest integer in 1..16 with 2^(2w) >= n (so 2^(2w) < 4 n), and perm(i) walks a balanced
 *   Feistel network P on 2w bits from x = i: x = P(x) until x < n (cycle walking: the walk follows a cycle of P that holds i < n, so it
 *   ends; a pass succeeds with probability n / 4^w > 1/4, the expected number of extra passes is below 3).
 *   P: (L, R) = (x >> w, x & (2^w - 1)); QR_SHUFFLE_ROUNDS = 8 rounds r = 0 .. 7 of (L, R) <- (R, L ^ F_r(R)); P(x) = L << w | R.
 *   F_r(v) = mix32(v + key[r]) >> (32 - w), the sum modulo 2^32, with the 32-bit multiply-xorshift finaliser
 *       mix32(x): x ^= x >> 16; x *= QR_SHUFFLE_MIX_M1; x ^= x >> 15; x *= QR_SHUFFLE_MIX_M2; x ^= x >> 16.
 *   key[4k .. 4k + 3] = the four raw Philox4x32-10 words of quad k of the qr_noise_fill stream for the triple
 *   seed, draw, stream (QrNoiseFill's counter layout; the words before they become floats).  A (seed, draw, stream) triple used here
 *   must not be used for a noise tensor as well.
 * Deviation from numpy / torch.randperm: another family of permutations (a keyed cipher, not Fisher-Yates or a sort of random keys),
 * and nothing is stored: element i costs a handful of passes wherever and whenever it is formed.
 * draw_dev: NULL, or one device int64 that the launch READS as the draw number (never written); `draw` is then ignored.
 * One launch: one thread per element, the grid min(ceil(count / 256), max_workgroups) with max_workgroups = 0: 1024, then strided —
 * the grid cannot change a value.  count = 0: nothing is launched (out may be NULL). */
#define QR_SHUFFLE_ROUNDS 8
#define QR_SHUFFLE_MIX_M1 0x7FEB352Du
#define QR_SHUFFLE_MIX_M2 0x846CA68Bu
typedef struct QrShuffle {
  int64_t* out;                   /* [count], written; 8-byte aligned */
  const int64_t* draw_dev;        /* NULL, or one device int64 that is READ as the draw number (never written) */
  int64_t n, first, count;        /* 1 <= n < 2^32; 0 <= first, 0 <= count, first + count <= n */
  uint64_t seed;
  int64_t draw;                   /* the draw number where draw_dev is NULL: >= 0 */
  uint32_t stream;                /* < 2^30 */
  int32_t max_workgroups;         /* 0: the library's choice (1024); > 0: a cap on the grid */
} QrShuffle;
/* In this order, all before the launch: QR_E_NULL for a NULL struct; QR_E_SIZE for n outside [1, 2^32), first < 0, count < 0,
 * first + count > n, a stream >= 2^30, max_workgroups < 0 or a negative draw where draw_dev is NULL; then count = 0 returns 0;
 * QR_E_NULL for a NULL out; QR_E_ALIGN for an out or draw_dev that is not 8-byte aligned.  Nothing is launched or written on an error. */
int qr_shuffle(const QrShuffle* shuffle, void* stream);

/* Host-side helpers (no device work). */
void qr_default_coeffs(QrCoeffs* c);
int  qr_abi_version(void);
/* What the launcher would run for this env — host-side, no device work; nothing in the reference (profilers, autotuners, tests).
 * qr_step / qr_rollout (actor = 0) or qr_rollout_actor (actor = 1: PPO / TD3-form actors, 2: the general form with SAC's
 * log_std head) over n_steps env-steps of `substeps` substeps: `launches` launches of `grid` workgroups (64-env tiles)
 * of `block` threads — 64 = one wavefront per tile, 128 = plus a helper wavefront (QR_FLAG_AUTO_RESET, default layout, grids
 * in the launch-latency regime; launches > 1: qr_rollout_actor in chunks of `grid` resident tiles) — of the instantiation
 * `name` = qr::step_kernel<KIND, XV, QW, 64, TRAJ, ADAPT, POLICY, SINGLE, HELP, HREW, MAG> with the values filled in (the prefix of
 * the kernel's name in a rocprofv3 trace; MAG = 1: the Magnus substep, substeps >= 2 in the default layout).  `key` = layout << 16 |
 * MAG << 12 | kind << 8 | TRAJ | ADAPT << 2 | POLICY << 3 | SINGLE << 5 | HELP << 6 | HREW << 7: what qr_launch_stats counts under. */
typedef struct QrLaunchPlan {
  int32_t grid, block, launches;
  int32_t traj, adapt, policy, single, help, hrew, mag;
  uint32_t key;
  char name[96];
} QrLaunchPlan;
int qr_launch_plan(const QrEnv* env, int32_t n_steps, int32_t substeps, int32_t actor, QrLaunchPlan* plan);
/* The older, shorter form: kernel family name + launch geometry of qr_step (n_steps = 1) / qr_rollout with ONE substep.
 * "" if the env descriptor is invalid. */
const char* qr_step_kernel_info(const QrEnv* env, int32_t n_steps, int32_t* grid, int32_t* block);
/* Host-side launch counters of this process: how many step-kernel launches each (layout, kind, instantiation) `key` has had
 * since load (or since the last call with reset != 0).  Writes up to `capacity` (key, count) pairs with count > 0, returns
 * how many there are.  qr_instance_table lists the keys of EVERY instantiation the library holds (175), same convention:
 * together they tell a test suite which kernels it really ran. */
int32_t qr_launch_stats(uint32_t* keys, uint32_t* counts, int32_t capacity, int32_t reset);
int32_t qr_instance_table(uint32_t* keys, int32_t capacity);

/* The step's memory traffic and nothing else: one launch that moves, per env, exactly what qr_step moves — state in and out,
 * parameters, the action row, [goal], [integrator words in and out], [observation rows], reward and done rows — with no
 * arithmetic.  The yardstick a step's time is priced against (bench.py: roofline.noop_kernel_us, measured live on the box
 * and the buffers of the run).  The env's state is written back as read, bit for bit; the output rows hold zeros afterwards. */
int qr_touch(const QrEnv* env, const float* action, const QrStepOut* out, void* stream);

/* The launch rule's thresholds in force in this process (compiled-in defaults or the QR_HELPER_GRID* environment variables), in
 * 64-env tiles: grids up to *step_quad (Quad-v0) / *step_wrappers (Coupled, Decoupled) tiles run qr_step with a helper wavefront
 * per tile, grids up to *rollout tiles run qr_rollout / qr_rollout_actor with one.  What a host-side autotuner needs to know
 * whether a grid is close enough to a crossover to be worth timing (QuadVecEnv: within +-25 %).  NULL pointers are skipped. */
void qr_launch_thresholds(int32_t* step_quad, int32_t* step_wrappers, int32_t* rollout);

#ifdef __cplusplus
}
#endif
#endif /* QUADROTOR_HIP_H */
