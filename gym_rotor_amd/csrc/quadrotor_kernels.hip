// quadrotor_kernels.hip — fused env.step() kernels for gfx950 (MI355X / CDNA4).
//
// One lane = one quadrotor.  A launch does, per env and per env-step, everything the
// reference's QuadEnv.step template does (gym_rotor/envs/quad.py:142-168):
//   action map / motor mixing -> S fixed RK4 substeps of the rigid-body ODE on
//   R^3 x R^3 x SO(3) x R^3 (quad.py:321-335) with zero-order-hold (f, M) -> error
//   observation + trapezoid integrators (quad.py:421-466) -> reward -> np.interp
//   normalisation -> done -> crash override [-> auto-reset].
//
// What bounds it: at N >= ~250 000 envs the bytes — the step streams its working set through the
// fabric at 67-73 % of the HBM roofline; at the metric's N = 65 536 (1024 tiles = one stepping wave per SIMD) the
// launch boundary (1.8 us between dependent kernels) plus the length of ONE wave's instruction stream, which a lone
// wave issues at one VALU instruction per ~5.6 cycles whatever its type.  So the design minimises BYTES per env and
// INSTRUCTIONS on the stepping wave's path:
//   * attitude is a unit quaternion integrated directly — q' = q (0,W)/2 is the same flow as R' = R hat(W) — and
//     stored as its smallest three components: the state is 12 words, not 18; R(q) is rebuilt in registers only
//     where the observation / reward needs it;
//   * x, v are stored as float32 and q, W as float64 in the default (mixed) layout; W is integrated and q accumulated
//     in float64, the RK4 stage quaternions are float32 (qr_dynamics.h);
//   * the whole working set stays in VGPRs across substeps and, in qr_rollout, across env-steps: HBM is touched once
//     in and once out;
//   * for grids small enough that every wave is resident at once, each tile gets a second, HELPER wavefront in the
//     same workgroup (HELP): it samples the tile's reset pool, forms Quad-v0's reward, samples the policy's noise
//     and carries observation rows out, in issue slots the lone stepping wave leaves empty;
//   * arguments are read so that scalar-cache misses on the kernarg segment (~0.4 us each) stay off the stepping
//     wave's critical path.
// Per-env SoA buffers are read/written with lane-contiguous accesses through buffer descriptors; caller-facing AoS
// rows (actions, observations) go through LDS so global traffic is linear 16-byte-per-lane stores.  The physics has
// no contraction larger than 3x3, so no MFMA there; the one real contraction on the path — the 16-wide PPO actor of
// qr_rollout_actor — does run on the matrix cores (qr_actor.h).
//
// Written directly for CDNA4: 64-lane wavefronts, one stepping wavefront per 64-env tile (N = 65 536 -> 1024
// workgroups = one per SIMD-32), workgroups of one or two wavefronts, 120-128 VGPRs for the Quad-v0 one-step kernels
// (four waves per SIMD at large N).
//
// Files (included in this order):
//   qr_args.h      kernel argument block, constants, per-env working set
//   qr_rng.h       Philox4x32-10, wave-cooperative reset draws, reset sampling
//   qr_dynamics.h  attitude helpers, quaternion-form RHS + RK4, row transposes, action maps, error obs
//   qr_traj.h      goal generator (trajectory_generator.py modes 0/1/6), SoA buffer accessor
//   qr_actor.h     PPO actor (MFMA / LDS forms), action sampling
//   qr_step.h      launch thresholds, Quad-v0 reward / termination, the helper wave, step_kernel (step / rollout)
//   qr_eval.h      batched policy evaluation (qr_evaluate_actor, qr_evaluate_population): eval_kernel
//   qr_aux.h       auxiliary kernels (error observation, reset, state get / set, goal generator), touch_kernel, gae_kernel
//   qr_critic.h    the PPO critic over a whole horizon (qr_critic_values, qr_critic_next_values): critic_kernel
//   qr_ppo.h       the PPO actor loss and its gradients for one minibatch (qr_ppo_actor_grad): ppo_actor_kernel, ppo_reduce_kernel
//   qr_mlp_grad.h  what the MLP-critic update kernels share (included by the next and by qr_td3.h): mlp_grad_walk, the gradient kernels' shared tile walk; the half-tile gradient body, the partial vector, the reduction's sums
//   qr_ppo_critic.h  the PPO critic loss and its gradients for one minibatch (qr_ppo_critic_grad): ppo_critic_kernel, ppo_critic_reduce_kernel
//   qr_optim.h     gradient-norm clipping, AdamW and the cosine schedule for up to eight parameter groups (qr_adamw_step): adamw_step_kernel;
//                  the same step for up to sixteen tensors with the soft target update and SAC's exp(log_alpha) fused (qr_adamw_polyak_step): adamw_polyak_kernel
//   qr_td3.h       the TD3 critic half for one minibatch (qr_twinq_target, qr_twinq_grad): td3_target_kernel, twinq_kernel, twinq_reduce_kernel; target_walk, the target kernels' shared tile walk;
//                  the centralized (CTDE) critic of two agents (qr_ctde_twinq_target, qr_ctde_sac_target, qr_ctde_twinq_grad): the walks' two-agent forms, ctde_twinq_kernel
//   qr_td3_actor.h the TD3 actor half for one minibatch and the soft target update (qr_dpg_actor_grad, qr_soft_update): dpg_actor_kernel, dpg_reduce_kernel, soft_update_kernel;
//                  agent k's actor half under the centralized (CTDE) critic (qr_ctde_dpg_actor_grad): the same walk's two-agent form, ctde_dpg_actor_kernel
//   qr_sac.h       SAC's soft target values for one minibatch (qr_sac_target): sac_sample, SacRule, sac_target_kernel
//   qr_sac_actor.h SAC's actor half for one minibatch (qr_sac_actor_grad): SacNet, SacRow, sac_actor_kernel, sac_actor_reduce_kernel;
//                  agent k's actor half under the centralized (CTDE) twin critic (qr_ctde_sac_actor_grad): ctde_sac_actor_kernel
//   qr_replay.h    the replay buffer's append and its minibatch indices (qr_replay_add, qr_replay_add_rule, qr_replay_sample):
//                  replay_add_kernel, replay_add_rule_kernel (the time-limit "solved" rule), replay_sample_kernel,
//                  replay_advance_kernel (the opt-in device counters)
//   qr_noise.h     the library's noise source (qr_noise_fill): up to sixteen normal or uniform tensors of a TD3 / SAC iteration from one
//                  counter-based stream in one launch: noise_fill_kernel
//   qr_shuffle.h   a keyed permutation of [0, n), PPO's epoch shuffle (qr_shuffle): a cycle-walking Feistel network under keys from the
//                  noise stream, no sort and no state: shuffle_kernel
//   qr_episode.h   the training curve from a collected horizon's rows (qr_episode_scan): per-episode return, length, end flags and final
//                  error, and their statistics: episode_scan_kernel, episode_reduce_kernel
//   qr_gae.h       PPO's advantages over the done flag the reference stores at the time limit, their per-agent statistics and their
//                  normalisation (qr_gae_rule): gae_rule_kernel, gae_fold_kernel, gae_normalize_kernel
//   qr_es.h        what surrounds the population evaluation in an evolution-strategy generation (qr_es_perturb, qr_es_gradient): the keyed
//                  antithetic perturbation, the fitness shaping and the gradient estimator: es_perturb_kernel, es_utility_kernel, es_grad_kernel
//   qr_launch.h    host side: argument blocks, the launch rule, the instantiation table, launchers
//   this file      the C-ABI; the launchers of the update entries, among them actor_grad_launch (qr_ppo_actor_grad, qr_dpg_actor_grad and qr_ctde_dpg_actor_grad),
//                  mlp_grad_launch (qr_ppo_critic_grad, qr_twinq_grad and qr_ctde_twinq_grad), target_launch (the four target entries) and
//                  sac_actor_launch (qr_sac_actor_grad and qr_ctde_sac_actor_grad), do_replay_add, do_replay_sample and do_episode_scan
// Build switches (the product build sets none): QR_SPAN, the light clock build (Makefile: span-lib); QR_ONLY_KIND /
// QR_ONLY_LAYOUT, developer builds with one env kind / one layout.  Settled A/Bs are constants in namespace qr (qr_step.h).
#include <hip/hip_runtime.h>
#include <initializer_list>
#include <stdio.h>
#include <string.h>
#include "quadrotor_hip.h"

#include "qr_args.h"
#include "qr_rng.h"
#include "qr_dynamics.h"
#include "qr_traj.h"
#include "qr_actor.h"
#include "qr_step.h"
#include "qr_eval.h"
#include "qr_aux.h"
#include "qr_critic.h"
#include "qr_ppo.h"
#include "qr_ppo_critic.h"
#include "qr_optim.h"
#include "qr_td3.h"
#include "qr_td3_actor.h"
#include "qr_sac.h"
#include "qr_sac_actor.h"
#include "qr_replay.h"
#include "qr_noise.h"
#include "qr_shuffle.h"
#include "qr_episode.h"
#include "qr_gae.h"
#include "qr_es.h"
#include "qr_launch.h"

namespace qr {
// Argument checks and the launch of both critic entry points; done = NULL: the values mode.
static int do_critic(const QrCritic* c, const float* rows0, const float* rows1, const uint8_t* done, int32_t n_agents, const uint8_t* truncated,
                     int64_t n_rows, int64_t n_envs, const float* value, float* out, int32_t stride, bool next, void* stream) {
  if (!c) return QR_E_NULL;
  if (c->in0 < 0 || c->in1 < 0 || c->in0 > kCriticIn || c->in1 > kCriticIn || c->in0 + c->in1 < 1 || c->in0 + c->in1 > kCriticIn) return QR_E_SIZE;
  if (c->hidden_dim < 1 || c->hidden_dim > 64 || n_rows < 0 || n_envs < 0 || stride < 1 || (next && n_agents < 1)) return QR_E_SIZE;
  if (!c->fc1_w || !c->fc1_b || !c->fc2_w || !c->fc2_b || !c->fc3_w || !c->fc3_b || !out) return QR_E_NULL;
  if ((c->in0 && !rows0) || (c->in1 && !rows1) || (next && (!done || !value))) return QR_E_NULL;
  const void* const floats[] = {c->fc1_w, c->fc1_b, c->fc2_w, c->fc2_b, c->fc3_w, c->fc3_b, rows0, rows1, value, out};
  for (const void* p : floats)
    if (reinterpret_cast<uintptr_t>(p) & 3u) return QR_E_ALIGN;
  if (n_rows == 0) return 0;
  const CriticArgs a{c->fc1_w, c->fc1_b, c->fc2_w, c->fc2_b, c->fc3_w, c->fc3_b, c->in0 ? rows0 : nullptr, c->in1 ? rows1 : nullptr,
                     done, truncated, value, out, n_rows, n_envs, c->in0, c->in1, c->hidden_dim, stride, n_agents};
  // grid-stride over the tiles: at most the waves that are resident at once, two per SIMD (256 CUs x 4 SIMDs x 2)
  const int64_t tiles = (n_rows + 63) / 64;
  const dim3 grid((unsigned)(tiles < 2048 ? tiles : 2048));
  if (next) hipLaunchKernelGGL(critic_kernel<true>, grid, dim3(64), 0, reinterpret_cast<hipStream_t>(stream), a);
  else hipLaunchKernelGGL(critic_kernel<false>, grid, dim3(64), 0, reinterpret_cast<hipStream_t>(stream), a);
  return (int)hipGetLastError();
}

// The grid of qr_ppo_actor_grad: a function of the batch and max_workgroups only (0: the waves resident at once, one per SIMD at
// the kernel's register count: 256 CUs x 4).
static int64_t ppo_grid(int64_t batch, int32_t max_workgroups) {
  const int64_t tiles = (batch + 63) / 64, cap = max_workgroups > 0 ? max_workgroups : 1024;
  return tiles < cap ? tiles : cap;
}

// Which of the rollout's three actor sizes (the index of every table over them); -1: none.
static int actor_size(int32_t d, int32_t h, int32_t a) {
  if (d == 23 && h == 16 && a == 4) return 0;
  if (d == 15 && h == 16 && a == 4) return 1;
  if (d == 3 && h == 4 && a == 1) return 2;
  return -1;
}
// length of a partial vector per actor size
constexpr int kPpoNP[3] = {PpoLayout<23, 16, 4>::NP, PpoLayout<15, 16, 4>::NP, PpoLayout<3, 4, 1>::NP};
constexpr int kDpgNP[3] = {DpgLayout<23, 16, 4>::NP, DpgLayout<15, 16, 4>::NP, DpgLayout<3, 4, 1>::NP};

// What qr_ppo_actor_grad and qr_dpg_actor_grad check, fill and launch alike; p and the caller's own structs are not NULL.  The caller
// has filled its own fields of `a` and `r` (among them a.index, a.partials = the workspace, a.B and a.lam_*) and says: whether the
// actor's log_std parameter is read, whether its own sizes and scalars are in range, whether its own pointers are there, its own
// float pointers, the gradient tensors in PpoLayout's order (7 or 6), the partial vector's length per actor size, its kernels for
// D = 23, 15, 3, and its reduce kernel with the entries one workgroup of it sums.
template <class Args, class RArgs>
static int actor_grad_launch(const QrActor* p, Args& a, RArgs& r, bool log_std, bool sizes_ok, bool supplied_ok, std::initializer_list<const void*> own,
                             float* const* grads, int n_grads, int64_t workspace_bytes, int32_t max_workgroups, const int (&np_of)[3],
                             void (*const kernel[3])(Args), void (*reduce)(RArgs), int per_workgroup, void* stream) {
  if (p->squash != QR_ACTOR_TANH_MEAN || p->log_std_w || p->log_std_b) return QR_E_KIND;
  const int size = actor_size(p->obs_dim, p->hidden_dim, p->action_dim);
  if (size < 0 || !sizes_ok || a.B < 1 || max_workgroups < 0) return QR_E_SIZE;
  if (!p->fc1_w || !p->fc1_b || !p->fc2_w || !p->fc2_b || !p->mean_w || !p->mean_b || (log_std && !p->log_std)) return QR_E_NULL;
  for (int k = 0; k < n_grads; ++k)
    if (!grads[k]) return QR_E_NULL;
  if (!a.partials || !supplied_ok) return QR_E_NULL;
  const void* const floats[] = {p->fc1_w, p->fc1_b, p->fc2_w, p->fc2_b, p->mean_w, p->mean_b, log_std ? p->log_std : nullptr};
  for (const void* q : floats)
    if (reinterpret_cast<uintptr_t>(q) & 3u) return QR_E_ALIGN;
  for (int k = 0; k < n_grads; ++k)
    if (reinterpret_cast<uintptr_t>(grads[k]) & 3u) return QR_E_ALIGN;
  for (const void* q : own)
    if (reinterpret_cast<uintptr_t>(q) & 3u) return QR_E_ALIGN;
  if ((reinterpret_cast<uintptr_t>(a.index) | reinterpret_cast<uintptr_t>(a.partials)) & 7u) return QR_E_ALIGN;
  const int64_t grid = ppo_grid(a.B, max_workgroups);
  const int np = np_of[size];
  if (workspace_bytes < grid * np * (int64_t)sizeof(double)) return QR_E_SIZE;

  const int D = p->obs_dim, H = p->hidden_dim, A = p->action_dim;
  const double B = (double)a.B, ba = B * A;
  // without log_std: PpoNet::fill copies action_dim floats from it into a slot the kernel never reads; mean_b is such an array
  a.w = ActorW{p->fc1_w, p->fc1_b, p->fc2_w, p->fc2_b, p->mean_w, p->mean_b, log_std ? p->log_std : p->mean_b, nullptr, nullptr, QR_ACTOR_TANH_MEAN};
  a.inv_b = (float)(1.0 / B); a.c_T = (float)(2.0 * a.lam_T / ba); a.c_S = (float)(2.0 * a.lam_S / ba); a.c_M = (float)(2.0 * a.lam_M / ba);
  const int sizes[7] = {H * D, H, H * H, H, A * H, A, A};
  r.partials = a.partials;
  for (int k = 0; k < n_grads; ++k) { r.grad[k] = grads[k]; r.off[k + 1] = r.off[k] + sizes[k]; }
  r.n_parts = (int32_t)grid; r.np = np;

  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(kernel[size], dim3((unsigned)grid), dim3(64), 0, s, a);
  if (int rc = (int)hipGetLastError()) return rc;
  hipLaunchKernelGGL(reduce, dim3((unsigned)((r.off[n_grads] + per_workgroup - 1) / per_workgroup + 1)), dim3(256), 0, s, r);
  return (int)hipGetLastError();
}

// entropy_coef_dev: NULL (qr_ppo_actor_grad), or the device float the reduce launch reads instead of b->entropy_coef
static int do_ppo_actor(const QrActor* c, const QrPpoBatch* b, const QrPpoGrad* g, const float* entropy_coef_dev, void* stream) {
  if (!c || !b || !g) return QR_E_NULL;
  const bool sizes_ok = b->n_steps >= 1 && b->n_envs >= 1 && b->row_stride >= 1 && b->adv_stride >= 1 && b->col_offset >= 0 &&
                        b->col_offset + c->action_dim <= b->row_stride && !(b->final_obs && b->n_agents < 1);
  const bool supplied_ok = g->stats && b->obs && b->action && b->logp_old && b->advantage && !(b->final_obs && !b->done) &&
                           !(b->lam_S != 0.0f && !b->noise) && !(b->lam_M != 0.0f && !b->nominal);
  PpoArgs a{};
  a.obs = b->obs; a.final_obs = b->final_obs; a.done = b->done; a.truncated = b->truncated;
  const int64_t col = sizes_ok && supplied_ok ? b->col_offset : 0;  // (no arithmetic on what the checks refuse)
  a.action = b->action + col; a.logp_old = b->logp_old + col; a.advantage = b->advantage; a.index = b->index;
  a.noise = b->lam_S != 0.0f ? b->noise : nullptr; a.nominal = b->lam_M != 0.0f ? b->nominal : nullptr;
  a.partials = static_cast<double*>(b->workspace);
  a.B = b->batch; a.N = b->n_envs; a.rows = (int64_t)b->n_steps * b->n_envs;
  a.act_stride = b->row_stride; a.adv_stride = b->adv_stride; a.n_agents = b->n_agents;
  a.clip = b->clip; a.max_action = b->max_action; a.lam_T = b->lam_T; a.lam_S = b->lam_S; a.lam_M = b->lam_M;
  PpoReduceArgs r{};
  r.stats = g->stats; r.log_std = c->log_std; r.action_dim = c->action_dim; r.B = (double)b->batch;
  r.entropy_coef = b->entropy_coef; r.entropy_coef_dev = entropy_coef_dev; r.lam_T = b->lam_T; r.lam_S = b->lam_S; r.lam_M = b->lam_M;
  float* const grads[7] = {g->fc1_w, g->fc1_b, g->fc2_w, g->fc2_b, g->mean_w, g->mean_b, g->log_std};
  static void (*const kernel[3])(PpoArgs) = {ppo_actor_kernel<23, 16, 4>, ppo_actor_kernel<15, 16, 4>, ppo_actor_kernel<3, 4, 1>};
  return actor_grad_launch(c, a, r, true, sizes_ok, supplied_ok,
                           {g->stats, b->obs, b->final_obs, b->action, b->logp_old, b->advantage, b->noise, b->nominal, entropy_coef_dev}, grads, 7,
                           b->workspace_bytes, b->max_workgroups, kPpoNP, kernel, ppo_reduce_kernel, 4, stream);
}

// The grid of an MLP-critic gradient launch (along x): a function of the batch and max_workgroups only.  0: default_cap, the waves
// resident at once, one per SIMD at the kernels' register count — 256 CUs x 4 = 1024 for qr_ppo_critic_grad (its 29 KB of LDS
// would admit five workgroups per CU), 512 for each of qr_twinq_grad's two rows.
static int64_t mlp_grad_grid(int64_t batch, int32_t max_workgroups, int64_t default_cap) {
  const int64_t tiles = (batch + 63) / 64, cap = max_workgroups > 0 ? max_workgroups : default_cap;
  return tiles < cap ? tiles : cap;
}
static int64_t ppo_critic_grid(int64_t batch, int32_t max_workgroups) { return mlp_grad_grid(batch, max_workgroups, 1024); }
static int64_t twinq_grid(int64_t batch, int32_t max_workgroups) { return mlp_grad_grid(batch, max_workgroups, 512); }

static bool ppo_critic_sizes_ok(int64_t in0, int64_t in1, int64_t hidden) {
  return in0 >= 0 && in1 >= 0 && in0 <= kCriticIn && in1 <= kCriticIn && in0 + in1 >= 1 && in0 + in1 <= kCriticIn && hidden >= 1 && hidden <= 64;
}

// What qr_ppo_critic_grad and qr_twinq_grad check, fill and launch alike; the caller's own structs are not NULL.  The caller has filled
// its own fields of `a` and `r` (among them a.index, a.partials = the workspace, a.B and r.grad) and says: whether its sizes are in range,
// whether its own pointers are there, its own float pointers, the gradient tensors (6 per network), the two input widths, the hidden
// width and the number of statistics, its grid rule, its workgroup rows (networks), and its two kernels.  The codes come in the order
// SIZE, NULL, ALIGN, the workspace's SIZE: what each entry returned before, which ordered its checks differently only inside one class.
template <class Args, class RArgs>
static int mlp_grad_launch(Args& a, RArgs& r, bool sizes_ok, bool supplied_ok, std::initializer_list<const void*> own, float* const* grads,
                           int in0, int in1, int H, int n_sums, int64_t (*grid_of)(int64_t, int32_t), int rows, int64_t workspace_bytes, int32_t max_workgroups,
                           void (*kernel)(Args), void (*reduce)(RArgs), void* stream) {
  if (!sizes_ok) return QR_E_SIZE;
  for (int k = 0; k < 6 * rows; ++k)
    if (!grads[k]) return QR_E_NULL;
  if (!supplied_ok) return QR_E_NULL;
  for (const void* q : own)
    if (reinterpret_cast<uintptr_t>(q) & 3u) return QR_E_ALIGN;
  for (int k = 0; k < 6 * rows; ++k)
    if (reinterpret_cast<uintptr_t>(grads[k]) & 3u) return QR_E_ALIGN;
  if ((reinterpret_cast<uintptr_t>(a.index) | reinterpret_cast<uintptr_t>(a.partials)) & 7u) return QR_E_ALIGN;
  const MlpGradLayout Y(in0 + in1, H, n_sums);
  const int64_t grid = grid_of(a.B, max_workgroups);
  if (workspace_bytes < rows * grid * Y.np * (int64_t)sizeof(double)) return QR_E_SIZE;
  a.g_scale = (float)(2.0 / (double)a.B);
  r.partials = a.partials; Y.starts(r.off); r.n_parts = (int32_t)grid; r.np = Y.np; r.B = (double)a.B;

  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid, (unsigned)rows), dim3(64), 0, s, a);
  if (int rc = (int)hipGetLastError()) return rc;
  hipLaunchKernelGGL(reduce, dim3((unsigned)((Y.st + 15) / 16 + 1), (unsigned)rows), dim3(256), 0, s, r);
  return (int)hipGetLastError();
}

static int do_ppo_critic(const QrCritic* c, const QrCriticBatch* b, const QrCriticGrad* g, void* stream) {
  if (!c || !b || !g) return QR_E_NULL;
  const bool sizes_ok = ppo_critic_sizes_ok(c->in0, c->in1, c->hidden_dim) && b->batch >= 1 && b->rows >= 1 && b->target_stride >= 1 && b->max_workgroups >= 0;
  const bool supplied_ok = c->fc1_w && c->fc1_b && c->fc2_w && c->fc2_b && c->fc3_w && c->fc3_b && g->stats && !(c->in0 && !b->obs0) &&
                           !(c->in1 && !b->obs1) && b->target && b->workspace;
  PpoCriticArgs a{};
  a.w = MlpNetW{c->fc1_w, c->fc1_b, c->fc2_w, c->fc2_b, c->fc3_w, c->fc3_b};
  a.rows0 = c->in0 ? b->obs0 : nullptr; a.rows1 = c->in1 ? b->obs1 : nullptr;
  a.target = b->target; a.index = b->index; a.partials = static_cast<double*>(b->workspace);
  a.B = b->batch; a.rows = b->rows; a.in0 = c->in0; a.in1 = c->in1; a.hidden = c->hidden_dim; a.tgt_stride = b->target_stride;
  PpoCriticReduceArgs r{};
  r.weight[0] = c->fc1_w; r.weight[1] = c->fc2_w; r.weight[2] = c->fc3_w;
  r.grad[0] = g->fc1_w; r.grad[1] = g->fc1_b; r.grad[2] = g->fc2_w; r.grad[3] = g->fc2_b; r.grad[4] = g->fc3_w; r.grad[5] = g->fc3_b;
  r.stats = g->stats; r.l2_reg = b->l2_reg;
  return mlp_grad_launch(a, r, sizes_ok, supplied_ok,
                         {c->fc1_w, c->fc1_b, c->fc2_w, c->fc2_b, c->fc3_w, c->fc3_b, g->stats, b->obs0, b->obs1, b->target}, r.grad,
                         c->in0, c->in1, c->hidden_dim, kPcSums, ppo_critic_grid, 1, b->workspace_bytes, b->max_workgroups,
                         ppo_critic_kernel, ppo_critic_reduce_kernel, stream);
}

static bool nonneg_finite(float v) { return v >= 0.0f && v <= 3.0e38f; }

static bool twinq_sizes_ok(int64_t obs_dim, int64_t action_dim, int64_t hidden) {
  return obs_dim >= 1 && action_dim >= 1 && obs_dim + action_dim <= TwinQL1::XS && hidden >= 1 && hidden <= 64;
}

static int twinq_critic_check(const QrQCritic* c) {  // sizes, then pointers, as every entry point orders them
  if (!twinq_sizes_ok(c->obs_dim, c->action_dim, c->hidden_dim) || c->reserved0 != 0) return QR_E_SIZE;
  if (!c->fc1_w || !c->fc1_b || !c->fc2_w || !c->fc2_b || !c->fc3_w || !c->fc3_b) return QR_E_NULL;
  if (!c->fc4_w || !c->fc4_b || !c->fc5_w || !c->fc5_b || !c->fc6_w || !c->fc6_b) return QR_E_NULL;
  return 0;
}

static void twinq_nets(MlpNetW (&n)[2], const QrQCritic* c) {
  n[0] = MlpNetW{c->fc1_w, c->fc1_b, c->fc2_w, c->fc2_b, c->fc3_w, c->fc3_b};
  n[1] = MlpNetW{c->fc4_w, c->fc4_b, c->fc5_w, c->fc5_b, c->fc6_w, c->fc6_b};
}

// The rows a target launch reads, from a QrTransitions (one agent: `two` false, [1] unused) or a QrCtdeTransitions.
struct TargetRows {
  const float* obs_next[2];
  const float *reward, *done;
  const int64_t* index;
  int64_t batch, rows;
  int32_t obs_dim[2], action_dim[2], reward_stride, done_stride;
  bool two;
};
static TargetRows target_rows(const QrQCritic* c, const QrTransitions* b) {
  return TargetRows{{b->obs_next, nullptr}, b->reward, b->done, b->index, b->batch, b->rows, {c->obs_dim, 0}, {c->action_dim, 0},
                    b->reward_stride, b->done_stride, false};
}
static TargetRows target_rows(const QrCtdeTransitions* b) {
  return TargetRows{{b->obs_next[0], b->obs_next[1]}, b->reward, b->done, b->index, b->batch, b->rows, {b->obs_dim[0], b->obs_dim[1]},
                    {b->action_dim[0], b->action_dim[1]}, b->reward_stride, b->done_stride, true};
}
// the four widths of a centralized critic's row: each >= 1, adding up to the critic's
static bool ctde_widths_ok(const QrQCritic* c, const int32_t (&od)[2], const int32_t (&ad)[2]) {
  return od[0] >= 1 && od[1] >= 1 && ad[0] >= 1 && ad[1] >= 1 && (int64_t)od[0] + od[1] == c->obs_dim && (int64_t)ad[0] + ad[1] == c->action_dim;
}

// What the four target entries check, fill and launch alike; c and the caller's own structs are not NULL.  p: the actor(s), both
// or neither in the centralized form.  The caller has filled its own fields of `a` and says: the actor form it takes (squash, log_std:
// with the log_std head), whether its scalars are in range, whether what the no-actor form reads is there, its own float pointers,
// and its kernels for AD = 23, 15, 3, 0 and the centralized form with both Decoupled actors and with none.
template <class Args>
static int target_launch(const QrActor* const (&p)[2], const QrQCritic* c, const TargetRows& b, Args& a, int32_t squash, bool log_std,
                         bool scalars_ok, bool supplied_ok, std::initializer_list<const void*> own, void (*const kernel[6])(Args), void* stream) {
  const int n = b.two ? 2 : 1;
  for (int m = 0; m < n; ++m)
    if (p[m] && (p[m]->squash != squash || (log_std ? !p[m]->log_std_w || !p[m]->log_std_b : p[m]->log_std_w || p[m]->log_std_b))) return QR_E_KIND;
  if (int rc = twinq_critic_check(c); rc == QR_E_SIZE) return rc;
  if (b.two) {
    if (!ctde_widths_ok(c, b.obs_dim, b.action_dim)) return QR_E_SIZE;
    if (p[0] && (actor_size(p[0]->obs_dim, p[0]->hidden_dim, p[0]->action_dim) != 1 || b.obs_dim[0] != 15 || b.action_dim[0] != 4)) return QR_E_SIZE;
    if (p[1] && (actor_size(p[1]->obs_dim, p[1]->hidden_dim, p[1]->action_dim) != 2 || b.obs_dim[1] != 3 || b.action_dim[1] != 1)) return QR_E_SIZE;
  } else if (p[0] && (actor_size(p[0]->obs_dim, p[0]->hidden_dim, p[0]->action_dim) < 0 || p[0]->obs_dim != c->obs_dim || p[0]->action_dim != c->action_dim)) {
    return QR_E_SIZE;
  }
  if (b.batch < 1 || b.rows < 1 || b.reward_stride < 1 || b.done_stride < 1) return QR_E_SIZE;
  if (!scalars_ok) return QR_E_SIZE;
  if (int rc = twinq_critic_check(c)) return rc;
  if (b.two && !p[0] != !p[1]) return QR_E_NULL;
  for (int m = 0; m < n; ++m)
    if (p[m] && (!p[m]->fc1_w || !p[m]->fc1_b || !p[m]->fc2_w || !p[m]->fc2_b || !p[m]->mean_w || !p[m]->mean_b)) return QR_E_NULL;
  if (!b.obs_next[0] || (b.two && !b.obs_next[1]) || !b.reward || !b.done || !a.y || (!p[0] && !supplied_ok)) return QR_E_NULL;
  const void* const floats[] = {c->fc1_w, c->fc1_b, c->fc2_w, c->fc2_b, c->fc3_w, c->fc3_b, c->fc4_w, c->fc4_b, c->fc5_w, c->fc5_b, c->fc6_w,
                                c->fc6_b, b.obs_next[0], b.obs_next[1], b.reward, b.done};
  for (const void* q : floats)
    if (reinterpret_cast<uintptr_t>(q) & 3u) return QR_E_ALIGN;
  for (int m = 0; m < n; ++m) {
    if (!p[m]) continue;
    const void* const w[] = {p[m]->fc1_w, p[m]->fc1_b, p[m]->fc2_w, p[m]->fc2_b, p[m]->mean_w, p[m]->mean_b, p[m]->log_std_w, p[m]->log_std_b};
    for (const void* q : w)
      if (reinterpret_cast<uintptr_t>(q) & 3u) return QR_E_ALIGN;
  }
  for (const void* q : own)
    if (reinterpret_cast<uintptr_t>(q) & 3u) return QR_E_ALIGN;
  if (reinterpret_cast<uintptr_t>(b.index) & 7u) return QR_E_ALIGN;

  for (int m = 0; m < n; ++m) {
    if (p[m]) a.actor[m] = ActorW{p[m]->fc1_w, p[m]->fc1_b, p[m]->fc2_w, p[m]->fc2_b, p[m]->mean_w, p[m]->mean_b, nullptr, p[m]->log_std_w, p[m]->log_std_b, squash};
    a.obs_next[m] = b.obs_next[m]; a.obs_dim[m] = b.obs_dim[m]; a.action_dim[m] = b.action_dim[m];
  }
  twinq_nets(a.net, c);
  a.reward = b.reward; a.done = b.done; a.index = b.index; a.B = b.batch; a.rows = b.rows;
  a.hidden = c->hidden_dim; a.rwd_stride = b.reward_stride; a.done_stride = b.done_stride;
  // grid-stride over the tiles: at most the waves resident at once, one per SIMD at the kernels' register count
  const int64_t tiles = (b.batch + 63) / 64;
  const dim3 grid((unsigned)(tiles < 1024 ? tiles : 1024));
  const int ad = p[0] ? p[0]->obs_dim : 0;
  const int which = b.two ? (p[0] ? 4 : 5) : ad == 23 ? 0 : ad == 15 ? 1 : ad == 3 ? 2 : 3;
  hipLaunchKernelGGL(kernel[which], grid, dim3(64), 0, reinterpret_cast<hipStream_t>(stream), a);
  return (int)hipGetLastError();
}

static bool td3_scalars_ok(float noise_clip, float max_action) { return nonneg_finite(noise_clip) && nonneg_finite(max_action); }
static void (*const kTd3TargetKernel[6])(Td3TargetArgs) = {td3_target_kernel<23>, td3_target_kernel<15>, td3_target_kernel<3>, td3_target_kernel<0>,
                                                           td3_target_kernel<15, 3>, td3_target_kernel<0, 0>};
static void (*const kSacTargetKernel[6])(SacTargetArgs) = {sac_target_kernel<23>, sac_target_kernel<15>, sac_target_kernel<3>, sac_target_kernel<0>,
                                                           sac_target_kernel<15, 3>, sac_target_kernel<0, 0>};

static int do_td3_target(const QrActor* p, const QrQCritic* c, const QrTransitions* b, const QrTd3Target* t, void* stream) {
  if (!c || !b || !t) return QR_E_NULL;
  Td3TargetArgs a{};
  a.eps[0] = p ? t->eps : nullptr; a.action_next[0] = p ? nullptr : t->action_next; a.y = t->y;
  a.discount = t->discount; a.target_noise = t->target_noise; a.noise_clip = t->noise_clip; a.max_action = t->max_action;
  return target_launch({p, nullptr}, c, target_rows(c, b), a, QR_ACTOR_TANH_MEAN, false, td3_scalars_ok(t->noise_clip, t->max_action),
                       t->action_next != nullptr, {t->eps, t->action_next, t->y}, kTd3TargetKernel, stream);
}

static int do_ctde_td3_target(const QrActor* p0, const QrActor* p1, const QrQCritic* c, const QrCtdeTransitions* b, const QrCtdeTd3Target* t, void* stream) {
  if (!c || !b || !t) return QR_E_NULL;
  const bool actors = p0 || p1;
  Td3TargetArgs a{};
  for (int m = 0; m < 2; ++m) { a.eps[m] = actors ? t->eps[m] : nullptr; a.action_next[m] = actors ? nullptr : t->action_next[m]; }
  a.y = t->y; a.discount = t->discount; a.target_noise = t->target_noise; a.noise_clip = t->noise_clip; a.max_action = t->max_action;
  return target_launch({p0, p1}, c, target_rows(b), a, QR_ACTOR_TANH_MEAN, false, td3_scalars_ok(t->noise_clip, t->max_action),
                       t->action_next[0] && t->action_next[1], {t->eps[0], t->eps[1], t->action_next[0], t->action_next[1], t->y},
                       kTd3TargetKernel, stream);
}

static int do_sac_target(const QrActor* p, const QrQCritic* c, const QrTransitions* b, const QrSacTarget* t, void* stream) {
  if (!c || !b || !t) return QR_E_NULL;
  SacTargetArgs a{};
  a.eps[0] = p ? t->eps : nullptr; a.action_next[0] = p ? nullptr : t->action_next; a.logp_next = p ? nullptr : t->logp_next;
  a.alpha_dev = t->alpha_dev; a.y = t->y; a.action_out[0] = t->action_out; a.logp_out = t->logp_out;
  a.discount = t->discount; a.alpha = t->alpha;
  return target_launch({p, nullptr}, c, target_rows(c, b), a, QR_ACTOR_TANH_SAMPLE, true, nonneg_finite(t->discount) && nonneg_finite(t->alpha),
                       t->action_next && t->logp_next, {t->eps, t->action_next, t->logp_next, t->alpha_dev, t->y, t->action_out, t->logp_out},
                       kSacTargetKernel, stream);
}

static int do_ctde_sac_target(const QrActor* p0, const QrActor* p1, const QrQCritic* c, const QrCtdeTransitions* b, const QrCtdeSacTarget* t, void* stream) {
  if (!c || !b || !t) return QR_E_NULL;
  const bool actors = p0 || p1;
  SacTargetArgs a{};
  for (int m = 0; m < 2; ++m) {
    a.eps[m] = actors ? t->eps[m] : nullptr; a.action_next[m] = actors ? nullptr : t->action_next[m]; a.action_out[m] = t->action_out[m];
  }
  a.eps_logp = actors ? t->eps_logp : nullptr; a.logp_next = actors ? nullptr : t->logp_next;
  a.alpha_dev = t->alpha_dev; a.y = t->y; a.logp_out = t->logp_out; a.discount = t->discount; a.alpha = t->alpha; a.own = t->agent;
  const bool scalars_ok = nonneg_finite(t->discount) && nonneg_finite(t->alpha) && (t->agent == 0 || t->agent == 1) && t->reserved0 == 0;
  return target_launch({p0, p1}, c, target_rows(b), a, QR_ACTOR_TANH_SAMPLE, true, scalars_ok,
                       t->action_next[0] && t->action_next[1] && t->logp_next,
                       {t->eps[0], t->eps[1], t->eps_logp, t->action_next[0], t->action_next[1], t->logp_next, t->alpha_dev, t->y, t->action_out[0],
                        t->action_out[1], t->logp_out}, kSacTargetKernel, stream);
}

static int do_twinq(const QrQCritic* c, const QrTransitions* b, const QrTwinQGrad* g, void* stream) {
  if (!c || !b || !g) return QR_E_NULL;
  const int critic = twinq_critic_check(c);
  const bool sizes_ok = critic != QR_E_SIZE && b->batch >= 1 && b->rows >= 1 && b->row_stride >= 1 && g->max_workgroups >= 0 && g->reserved0 == 0 &&
                        b->col_offset >= 0 && b->col_offset + c->action_dim <= b->row_stride;
  const bool supplied_ok = critic == 0 && g->stats && g->y && g->workspace && b->obs && b->action;
  TwinQArgs a{};
  twinq_nets(a.net, c);
  const int64_t col = sizes_ok && supplied_ok ? b->col_offset : 0;  // (no arithmetic on what the checks refuse)
  a.obs = b->obs; a.action = b->action + col; a.y = g->y; a.index = b->index; a.partials = static_cast<double*>(g->workspace);
  a.B = b->batch; a.rows = b->rows; a.obs_dim = c->obs_dim; a.action_dim = c->action_dim; a.hidden = c->hidden_dim; a.act_stride = b->row_stride;
  TwinQReduceArgs r{};
  float* const grads[12] = {g->fc1_w, g->fc1_b, g->fc2_w, g->fc2_b, g->fc3_w, g->fc3_b, g->fc4_w, g->fc4_b, g->fc5_w, g->fc5_b, g->fc6_w, g->fc6_b};
  for (int k = 0; k < 12; ++k) r.grad[k / 6][k % 6] = grads[k];
  r.stats = g->stats;
  return mlp_grad_launch(a, r, sizes_ok, supplied_ok,
                         {c->fc1_w, c->fc1_b, c->fc2_w, c->fc2_b, c->fc3_w, c->fc3_b, c->fc4_w, c->fc4_b, c->fc5_w, c->fc5_b, c->fc6_w, c->fc6_b,
                          g->stats, g->y, b->obs, b->action}, grads,
                         c->obs_dim, c->action_dim, c->hidden_dim, kTqSums, twinq_grid, 2, g->workspace_bytes, g->max_workgroups,
                         twinq_kernel, twinq_reduce_kernel, stream);
}

// qr_twinq_grad's checks, launcher, grid and reduction; the kernel's rule stages four sources.
static int do_ctde_twinq(const QrQCritic* c, const QrCtdeTransitions* b, const QrTwinQGrad* g, void* stream) {
  if (!c || !b || !g) return QR_E_NULL;
  const int critic = twinq_critic_check(c);
  bool sizes_ok = critic != QR_E_SIZE && ctde_widths_ok(c, b->obs_dim, b->action_dim) && b->batch >= 1 && b->rows >= 1 && g->max_workgroups >= 0 &&
                  g->reserved0 == 0;
  for (int m = 0; m < 2; ++m)
    sizes_ok = sizes_ok && b->row_stride[m] >= 1 && b->col_offset[m] >= 0 && (int64_t)b->col_offset[m] + b->action_dim[m] <= b->row_stride[m];
  const bool supplied_ok = critic == 0 && g->stats && g->y && g->workspace && b->obs[0] && b->obs[1] && b->action[0] && b->action[1];
  CtdeTwinQArgs a{};
  twinq_nets(a.net, c);
  for (int m = 0; m < 2; ++m) {
    const int64_t col = sizes_ok && supplied_ok ? b->col_offset[m] : 0;  // (no arithmetic on what the checks refuse)
    a.obs[m] = b->obs[m]; a.action[m] = b->action[m] + col;
    a.obs_dim[m] = b->obs_dim[m]; a.action_dim[m] = b->action_dim[m]; a.act_stride[m] = b->row_stride[m];
  }
  a.y = g->y; a.index = b->index; a.partials = static_cast<double*>(g->workspace); a.B = b->batch; a.rows = b->rows; a.hidden = c->hidden_dim;
  TwinQReduceArgs r{};
  float* const grads[12] = {g->fc1_w, g->fc1_b, g->fc2_w, g->fc2_b, g->fc3_w, g->fc3_b, g->fc4_w, g->fc4_b, g->fc5_w, g->fc5_b, g->fc6_w, g->fc6_b};
  for (int k = 0; k < 12; ++k) r.grad[k / 6][k % 6] = grads[k];
  r.stats = g->stats;
  return mlp_grad_launch(a, r, sizes_ok, supplied_ok,
                         {c->fc1_w, c->fc1_b, c->fc2_w, c->fc2_b, c->fc3_w, c->fc3_b, c->fc4_w, c->fc4_b, c->fc5_w, c->fc5_b, c->fc6_w, c->fc6_b,
                          g->stats, g->y, b->obs[0], b->obs[1], b->action[0], b->action[1]}, grads,
                         c->obs_dim, c->action_dim, c->hidden_dim, kTqSums, twinq_grid, 2, g->workspace_bytes, g->max_workgroups,
                         ctde_twinq_kernel, twinq_reduce_kernel, stream);
}

// (the grid of qr_dpg_actor_grad is ppo_grid's: one wave per SIMD at the kernel's register count, 256 CUs x 4)
static int do_dpg_actor(const QrActor* p, const QrQCritic* c, const QrTransitions* b, const QrDpgGrad* g, void* stream) {
  if (!p || !c || !b || !g) return QR_E_NULL;
  const bool sizes_ok = twinq_sizes_ok(c->obs_dim, c->action_dim, c->hidden_dim) && c->reserved0 == 0 && p->obs_dim == c->obs_dim &&
                        p->action_dim == c->action_dim && b->rows >= 1 && g->reserved0 == 0 && nonneg_finite(g->max_action) &&
                        nonneg_finite(g->lam_T) && nonneg_finite(g->lam_S) && nonneg_finite(g->lam_M);
  const bool supplied_ok = c->fc1_w && c->fc1_b && c->fc2_w && c->fc2_b && c->fc3_w && c->fc3_b && g->stats && b->obs &&  // (Q2 is not read)
                           !(g->lam_T != 0.0f && !b->obs_next) && !(g->lam_S != 0.0f && !g->noise) && !(g->lam_M != 0.0f && !g->nominal);
  DpgArgs a{};
  a.q = MlpNetW{c->fc1_w, c->fc1_b, c->fc2_w, c->fc2_b, c->fc3_w, c->fc3_b};
  a.obs = b->obs; a.obs_next = g->lam_T != 0.0f ? b->obs_next : nullptr; a.index = b->index;
  a.noise = g->lam_S != 0.0f ? g->noise : nullptr; a.nominal = g->lam_M != 0.0f ? g->nominal : nullptr;
  a.partials = static_cast<double*>(g->workspace);
  a.B = b->batch; a.rows = b->rows; a.hidden = c->hidden_dim; a.max_action = g->max_action;
  a.lam_T = g->lam_T; a.lam_S = g->lam_S; a.lam_M = g->lam_M;
  DpgReduceArgs r{};
  r.stats = g->stats; r.B = (double)b->batch; r.BA = r.B * p->action_dim; r.lam_T = g->lam_T; r.lam_S = g->lam_S; r.lam_M = g->lam_M;
  float* const grads[6] = {g->fc1_w, g->fc1_b, g->fc2_w, g->fc2_b, g->mean_w, g->mean_b};
  static void (*const kernel[3])(DpgArgs) = {dpg_actor_kernel<23, 16, 4>, dpg_actor_kernel<15, 16, 4>, dpg_actor_kernel<3, 4, 1>};
  return actor_grad_launch(p, a, r, false, sizes_ok, supplied_ok,
                           {c->fc1_w, c->fc1_b, c->fc2_w, c->fc2_b, c->fc3_w, c->fc3_b, g->stats, g->noise, g->nominal, b->obs, b->obs_next}, grads, 6,
                           g->workspace_bytes, g->max_workgroups, kDpgNP, kernel, dpg_reduce_kernel, 16, stream);
}

// qr_dpg_actor_grad's launcher, grid, partial vector and reduction for agent k of two under one centralized critic.  actor_grad_launch
// fits: it is given agent k's actor, and what is this entry's own arrives in its classes — the other actor's form first (KIND comes
// first there too), the widths, the pair's sizes and `agent` in sizes_ok, the form's pointers in supplied_ok, the other actor's
// tensors among `own` for the alignment.  The table's first place (the 23-wide actor) is empty: 23 + 1 + 4 + 1 > 28, refused above.
static int do_ctde_dpg_actor(const QrActor* p0, const QrActor* p1, const QrQCritic* c, const QrCtdeTransitions* b, const QrCtdeDpgGrad* g, void* stream) {
  if (!c || !b || !g) return QR_E_NULL;
  const QrActor* const p[2] = {p0, p1};
  for (int m = 0; m < 2; ++m)
    if (p[m] && (p[m]->squash != QR_ACTOR_TANH_MEAN || p[m]->log_std_w || p[m]->log_std_b)) return QR_E_KIND;
  if (p0 && p1 && g->action_other) return QR_E_KIND;
  if (g->agent != 0 && g->agent != 1) return QR_E_SIZE;
  const int k = g->agent;
  const QrActor *own = p[k], *other = p[1 - k];
  bool sizes_ok = twinq_sizes_ok(c->obs_dim, c->action_dim, c->hidden_dim) && c->reserved0 == 0 && ctde_widths_ok(c, b->obs_dim, b->action_dim) &&
                  b->batch >= 1 && b->rows >= 1 && g->max_workgroups >= 0 && g->reserved0 == 0 && g->reserved1 == 0 && nonneg_finite(g->max_action) &&
                  nonneg_finite(g->lam_T) && nonneg_finite(g->lam_S) && nonneg_finite(g->lam_M);
  if (own) sizes_ok = sizes_ok && actor_size(own->obs_dim, own->hidden_dim, own->action_dim) == 1 + k && own->obs_dim == b->obs_dim[k] && own->action_dim == b->action_dim[k];
  if (other) sizes_ok = sizes_ok && actor_size(other->obs_dim, other->hidden_dim, other->action_dim) == 2 - k && other->obs_dim == b->obs_dim[1 - k] &&
                        other->action_dim == b->action_dim[1 - k];
  if (!sizes_ok) return QR_E_SIZE;
  if (!own) return QR_E_NULL;
  const bool other_ok = other ? other->fc1_w && other->fc1_b && other->fc2_w && other->fc2_b && other->mean_w && other->mean_b : g->action_other != nullptr;
  const bool supplied_ok = other_ok && c->fc1_w && c->fc1_b && c->fc2_w && c->fc2_b && c->fc3_w && c->fc3_b && g->stats && b->obs[0] && b->obs[1] &&  // (Q2 is not read)
                           !(g->lam_T != 0.0f && !b->obs_next[k]) && !(g->lam_S != 0.0f && !g->noise) && !(g->lam_M != 0.0f && !g->nominal);
  CtdeDpgArgs a{};
  a.q = MlpNetW{c->fc1_w, c->fc1_b, c->fc2_w, c->fc2_b, c->fc3_w, c->fc3_b};
  a.obs = b->obs[k]; a.obs_next = g->lam_T != 0.0f ? b->obs_next[k] : nullptr; a.index = b->index;
  a.noise = g->lam_S != 0.0f ? g->noise : nullptr; a.nominal = g->lam_M != 0.0f ? g->nominal : nullptr;
  a.partials = static_cast<double*>(g->workspace);
  a.B = b->batch; a.rows = b->rows; a.hidden = c->hidden_dim; a.max_action = g->max_action;
  a.lam_T = g->lam_T; a.lam_S = g->lam_S; a.lam_M = g->lam_M;
  if (other) a.other = ActorW{other->fc1_w, other->fc1_b, other->fc2_w, other->fc2_b, other->mean_w, other->mean_b, other->mean_b, nullptr, nullptr, QR_ACTOR_TANH_MEAN};  // (log_std: as in actor_grad_launch)
  a.obs_other = b->obs[1 - k]; a.action_other = other ? nullptr : g->action_other;
  a.od_other = b->obs_dim[1 - k]; a.ad_other = b->action_dim[1 - k];
  a.col_own = k ? b->obs_dim[0] : 0; a.col_other = k ? 0 : b->obs_dim[0];
  a.acol_own = c->obs_dim + (k ? b->action_dim[0] : 0); a.acol_other = c->obs_dim + (k ? 0 : b->action_dim[0]);
  a.in_dim = c->obs_dim + c->action_dim;
  DpgReduceArgs r{};
  r.stats = g->stats; r.B = (double)b->batch; r.BA = r.B * own->action_dim; r.lam_T = g->lam_T; r.lam_S = g->lam_S; r.lam_M = g->lam_M;
  float* const grads[6] = {g->fc1_w, g->fc1_b, g->fc2_w, g->fc2_b, g->mean_w, g->mean_b};
  static void (*const kernel[3])(CtdeDpgArgs) = {nullptr, ctde_dpg_actor_kernel<15, 16, 4>, ctde_dpg_actor_kernel<3, 4, 1>};
  const float *o1 = other ? other->fc1_w : nullptr, *o2 = other ? other->fc1_b : nullptr, *o3 = other ? other->fc2_w : nullptr,
              *o4 = other ? other->fc2_b : nullptr, *o5 = other ? other->mean_w : nullptr, *o6 = other ? other->mean_b : nullptr;
  return actor_grad_launch(own, a, r, false, true, supplied_ok,
                           {c->fc1_w, c->fc1_b, c->fc2_w, c->fc2_b, c->fc3_w, c->fc3_b, g->stats, g->noise, g->nominal, b->obs[0], b->obs[1],
                            b->obs_next[k], g->action_other, o1, o2, o3, o4, o5, o6}, grads, 6,
                           g->workspace_bytes, g->max_workgroups, kDpgNP, kernel, dpg_reduce_kernel, 16, stream);
}

constexpr int kSacNP[3] = {SacLayout<23, 16, 4>::NP, SacLayout<15, 16, 4>::NP, SacLayout<3, 4, 1>::NP};

// What qr_sac_actor_grad and qr_ctde_sac_actor_grad check last, fill and launch alike: the alignment, the workspace's size, the
// fields of `a` and of the reduction that come from the actor p (the one that gets gradients), the critic and QrSacActorGrad's members,
// and the two launches on ppo_grid's grid.  The caller has made its KIND, SIZE and NULL checks, filled a.obs, a.obs_next, a.index, a.B,
// a.rows and the fields of its own form, and hands its own float pointers for the alignment and its kernels per actor size.
template <class Args>
static int sac_actor_launch(const QrActor* p, const QrQCritic* c, const QrSacActorGrad* g, Args& a, std::initializer_list<const void*> own,
                            void (*const kernel[3])(Args), void* stream) {
  float* const grads[8] = {g->fc1_w, g->fc1_b, g->fc2_w, g->fc2_b, g->mean_w, g->mean_b, g->log_std_w, g->log_std_b};
  const void* const floats[] = {p->fc1_w, p->fc1_b, p->fc2_w, p->fc2_b, p->mean_w, p->mean_b, p->log_std_w, p->log_std_b, c->fc1_w, c->fc1_b,
                                c->fc2_w, c->fc2_b, c->fc3_w, c->fc3_b, c->fc4_w, c->fc4_b, c->fc5_w, c->fc5_b, c->fc6_w, c->fc6_b, g->fc1_w,
                                g->fc1_b, g->fc2_w, g->fc2_b, g->mean_w, g->mean_b, g->log_std_w, g->log_std_b, g->stats, g->eps, g->eps_reg,
                                g->eps_next, g->eps_pert, g->noise, g->nominal, g->alpha_dev, g->alpha_grad};
  for (const void* q : floats)
    if (reinterpret_cast<uintptr_t>(q) & 3u) return QR_E_ALIGN;
  for (const void* q : own)
    if (reinterpret_cast<uintptr_t>(q) & 3u) return QR_E_ALIGN;
  if ((reinterpret_cast<uintptr_t>(a.index) | reinterpret_cast<uintptr_t>(g->workspace)) & 7u) return QR_E_ALIGN;
  const int size = actor_size(p->obs_dim, p->hidden_dim, p->action_dim);
  const int64_t grid = ppo_grid(a.B, g->max_workgroups);
  const int np = kSacNP[size];
  if (g->workspace_bytes < grid * np * (int64_t)sizeof(double)) return QR_E_SIZE;

  const int D = p->obs_dim, H = p->hidden_dim, A = p->action_dim;
  const double B = (double)a.B, ba = B * A;
  // (PpoNet::fill copies action_dim floats from log_std into a slot this kernel never reads; mean_b is such an array)
  a.w = ActorW{p->fc1_w, p->fc1_b, p->fc2_w, p->fc2_b, p->mean_w, p->mean_b, p->mean_b, p->log_std_w, p->log_std_b, QR_ACTOR_TANH_SAMPLE};
  twinq_nets(a.q, c);
  const bool any = g->lam_T != 0.0f || g->lam_S != 0.0f || g->lam_M != 0.0f;
  a.eps[0] = g->eps; a.eps[1] = any ? g->eps_reg : nullptr; a.eps[2] = g->lam_T != 0.0f ? g->eps_next : nullptr;
  a.eps[3] = g->lam_S != 0.0f ? g->eps_pert : nullptr;
  a.noise = g->lam_S != 0.0f ? g->noise : nullptr; a.nominal = g->lam_M != 0.0f ? g->nominal : nullptr;
  a.alpha_dev = g->alpha_dev; a.partials = static_cast<double*>(g->workspace);
  a.hidden = c->hidden_dim; a.alpha = g->alpha; a.max_action = g->max_action;
  a.lam_T = g->lam_T; a.lam_S = g->lam_S; a.lam_M = g->lam_M;
  a.inv_b = (float)(1.0 / B); a.c_T = (float)(2.0 * a.lam_T / ba); a.c_S = (float)(2.0 * a.lam_S / ba); a.c_M = (float)(2.0 * a.lam_M / ba);
  SacActorReduceArgs r{};
  const int sizes[8] = {H * D, H, H * H, H, A * H, A, A * H, A};
  r.partials = a.partials;
  for (int k = 0; k < 8; ++k) { r.grad[k] = grads[k]; r.off[k + 1] = r.off[k] + sizes[k]; }
  r.stats = g->stats; r.alpha_grad = g->alpha_grad; r.alpha_dev = g->alpha_dev; r.n_parts = (int32_t)grid; r.np = np; r.B = B; r.BA = ba;
  r.alpha = g->alpha; r.target_entropy = g->target_entropy; r.lam_T = g->lam_T; r.lam_S = g->lam_S; r.lam_M = g->lam_M;

  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(kernel[size], dim3((unsigned)grid), dim3(64), 0, s, a);
  if (int rc = (int)hipGetLastError()) return rc;
  hipLaunchKernelGGL(sac_actor_reduce_kernel, dim3((unsigned)((r.off[8] + 15) / 16 + 1)), dim3(256), 0, s, r);
  return (int)hipGetLastError();
}

// (actor_grad_launch does not fit: it takes the tanh-of-mean form with six or seven tensors and no second critic; the order of the
//  checks is its own — KIND, SIZE, NULL, ALIGN, the workspace's SIZE — and the grid is ppo_grid's)
static int do_sac_actor(const QrActor* p, const QrQCritic* c, const QrTransitions* b, const QrSacActorGrad* g, void* stream) {
  if (!p || !c || !b || !g) return QR_E_NULL;
  if (p->squash != QR_ACTOR_TANH_SAMPLE || !p->log_std_w || !p->log_std_b) return QR_E_KIND;
  const int size = actor_size(p->obs_dim, p->hidden_dim, p->action_dim);
  if (size < 0 || !twinq_sizes_ok(c->obs_dim, c->action_dim, c->hidden_dim) || c->reserved0 != 0 || p->obs_dim != c->obs_dim ||
      p->action_dim != c->action_dim || b->batch < 1 || b->rows < 1 || g->reserved0 != 0 || g->max_workgroups < 0 || !nonneg_finite(g->alpha) ||
      !nonneg_finite(g->max_action) || !nonneg_finite(g->lam_T) || !nonneg_finite(g->lam_S) || !nonneg_finite(g->lam_M) ||
      !(g->target_entropy >= -3.0e38f && g->target_entropy <= 3.0e38f))
    return QR_E_SIZE;
  if (int rc = twinq_critic_check(c)) return rc;
  if (!p->fc1_w || !p->fc1_b || !p->fc2_w || !p->fc2_b || !p->mean_w || !p->mean_b) return QR_E_NULL;
  float* const grads[8] = {g->fc1_w, g->fc1_b, g->fc2_w, g->fc2_b, g->mean_w, g->mean_b, g->log_std_w, g->log_std_b};
  for (float* q : grads)
    if (!q) return QR_E_NULL;
  if (!g->stats || !g->workspace || !b->obs || (g->lam_T != 0.0f && !b->obs_next) || (g->lam_S != 0.0f && !g->noise) ||
      (g->lam_M != 0.0f && !g->nominal))
    return QR_E_NULL;
  SacActorArgs a{};
  a.obs = b->obs; a.obs_next = g->lam_T != 0.0f ? b->obs_next : nullptr; a.index = b->index; a.B = b->batch; a.rows = b->rows;
  static void (*const kernel[3])(SacActorArgs) = {sac_actor_kernel<23, 16, 4>, sac_actor_kernel<15, 16, 4>, sac_actor_kernel<3, 4, 1>};
  return sac_actor_launch(p, c, g, a, {b->obs, b->obs_next}, kernel, stream);
}

// qr_sac_actor_grad's launcher, grid, partial vector and reduction for agent k of two under one centralized twin critic.  The checks
// come in qr_ctde_dpg_actor_grad's order with SAC's actor form; the grad struct's leading members are QrSacActorGrad's (checked below),
// so sac_actor_launch reads them as one.  The table's first place (the 23-wide actor) is empty: 23 + 1 + 4 + 1 > 28, refused above.
static_assert(offsetof(QrCtdeSacActorGrad, reserved0) == offsetof(QrSacActorGrad, reserved0) &&
              offsetof(QrCtdeSacActorGrad, workspace_bytes) == offsetof(QrSacActorGrad, workspace_bytes) &&
              offsetof(QrCtdeSacActorGrad, agent) == sizeof(QrSacActorGrad), "QrCtdeSacActorGrad begins with QrSacActorGrad's members");
static int do_ctde_sac_actor(const QrActor* p0, const QrActor* p1, const QrQCritic* c, const QrCtdeTransitions* b, const QrCtdeSacActorGrad* g,
                             void* stream) {
  if (!c || !b || !g) return QR_E_NULL;
  const QrActor* const p[2] = {p0, p1};
  for (int m = 0; m < 2; ++m)
    if (p[m] && (p[m]->squash != QR_ACTOR_TANH_SAMPLE || !p[m]->log_std_w || !p[m]->log_std_b)) return QR_E_KIND;
  if (p0 && p1 && g->action_other) return QR_E_KIND;
  if (g->agent != 0 && g->agent != 1) return QR_E_SIZE;
  const int k = g->agent;
  const QrActor *own = p[k], *other = p[1 - k];
  bool sizes_ok = twinq_sizes_ok(c->obs_dim, c->action_dim, c->hidden_dim) && c->reserved0 == 0 && ctde_widths_ok(c, b->obs_dim, b->action_dim) &&
                  b->batch >= 1 && b->rows >= 1 && g->max_workgroups >= 0 && g->reserved0 == 0 && g->reserved1 == 0 && nonneg_finite(g->alpha) &&
                  nonneg_finite(g->max_action) && nonneg_finite(g->lam_T) && nonneg_finite(g->lam_S) && nonneg_finite(g->lam_M) &&
                  g->target_entropy >= -3.0e38f && g->target_entropy <= 3.0e38f;
  if (own) sizes_ok = sizes_ok && actor_size(own->obs_dim, own->hidden_dim, own->action_dim) == 1 + k && own->obs_dim == b->obs_dim[k] && own->action_dim == b->action_dim[k];
  if (other) sizes_ok = sizes_ok && actor_size(other->obs_dim, other->hidden_dim, other->action_dim) == 2 - k && other->obs_dim == b->obs_dim[1 - k] &&
                        other->action_dim == b->action_dim[1 - k];
  if (!sizes_ok) return QR_E_SIZE;
  if (!own) return QR_E_NULL;
  if (other ? !other->fc1_w || !other->fc1_b || !other->fc2_w || !other->fc2_b || !other->mean_w || !other->mean_b : !g->action_other) return QR_E_NULL;
  if (int rc = twinq_critic_check(c)) return rc;
  if (!own->fc1_w || !own->fc1_b || !own->fc2_w || !own->fc2_b || !own->mean_w || !own->mean_b) return QR_E_NULL;
  float* const grads[8] = {g->fc1_w, g->fc1_b, g->fc2_w, g->fc2_b, g->mean_w, g->mean_b, g->log_std_w, g->log_std_b};
  for (float* q : grads)
    if (!q) return QR_E_NULL;
  if (!g->stats || !g->workspace || !b->obs[0] || !b->obs[1] || (g->lam_T != 0.0f && !b->obs_next[k]) || (g->lam_S != 0.0f && !g->noise) ||
      (g->lam_M != 0.0f && !g->nominal))
    return QR_E_NULL;
  CtdeSacActorArgs a{};
  a.obs = b->obs[k]; a.obs_next = g->lam_T != 0.0f ? b->obs_next[k] : nullptr; a.index = b->index; a.B = b->batch; a.rows = b->rows;
  // (log_std: as in sac_actor_launch)
  if (other) a.other = ActorW{other->fc1_w, other->fc1_b, other->fc2_w, other->fc2_b, other->mean_w, other->mean_b, other->mean_b, other->log_std_w,
                              other->log_std_b, QR_ACTOR_TANH_SAMPLE};
  a.obs_other = b->obs[1 - k]; a.action_other = other ? nullptr : g->action_other; a.eps_other = other ? g->eps_other : nullptr;
  a.eps_logp = g->eps_logp;
  a.od_other = b->obs_dim[1 - k]; a.ad_other = b->action_dim[1 - k];
  a.col_own = k ? b->obs_dim[0] : 0; a.col_other = k ? 0 : b->obs_dim[0];
  a.acol_own = c->obs_dim + (k ? b->action_dim[0] : 0); a.acol_other = c->obs_dim + (k ? 0 : b->action_dim[0]);
  a.in_dim = c->obs_dim + c->action_dim;
  static void (*const kernel[3])(CtdeSacActorArgs) = {nullptr, ctde_sac_actor_kernel<15, 16, 4>, ctde_sac_actor_kernel<3, 4, 1>};
  const float *o1 = other ? other->fc1_w : nullptr, *o2 = other ? other->fc1_b : nullptr, *o3 = other ? other->fc2_w : nullptr,
              *o4 = other ? other->fc2_b : nullptr, *o5 = other ? other->mean_w : nullptr, *o6 = other ? other->mean_b : nullptr,
              *o7 = other ? other->log_std_w : nullptr, *o8 = other ? other->log_std_b : nullptr;
  return sac_actor_launch(own, c, reinterpret_cast<const QrSacActorGrad*>(g), a,
                          {b->obs[0], b->obs[1], b->obs_next[k], g->eps_logp, g->eps_other, g->action_other, o1, o2, o3, o4, o5, o6, o7, o8}, kernel, stream);
}

static int do_soft_update(const QrSoftUpdate* u, void* stream) {
  if (!u) return QR_E_NULL;
  if (u->n_tensors < 1 || u->n_tensors > kSoftMax || u->reserved0 != 0 || !(u->tau >= 0.0 && u->tau <= 1.0)) return QR_E_SIZE;
  for (int k = 0; k < u->n_tensors; ++k)
    if (u->count[k] < 1) return QR_E_SIZE;
  for (int k = 0; k < u->n_tensors; ++k)
    if (!u->target[k] || !u->param[k]) return QR_E_NULL;
  for (int k = 0; k < u->n_tensors; ++k)
    if (u->target[k] == u->param[k]) return QR_E_SIZE;
  for (int k = 0; k < u->n_tensors; ++k)
    if ((reinterpret_cast<uintptr_t>(u->target[k]) | reinterpret_cast<uintptr_t>(u->param[k])) & 3u) return QR_E_ALIGN;
  SoftUpdateArgs a{};
  int64_t widest = 0;
  for (int k = 0; k < u->n_tensors; ++k) {
    a.target[k] = u->target[k]; a.param[k] = u->param[k]; a.count[k] = u->count[k];
    widest = u->count[k] > widest ? u->count[k] : widest;
  }
  a.tau = (float)u->tau; a.omt = (float)(1.0 - u->tau);
  const int64_t cols = (widest + 255) / 256;
  hipLaunchKernelGGL(soft_update_kernel, dim3((unsigned)(cols < kSoftCols ? cols : kSoftCols), (unsigned)u->n_tensors), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  return (int)hipGetLastError();
}

// ceil(2^32 / w) for w >= 2: what replay_add_kernel splits a tile offset into (row, column) with
static uint32_t replay_magic(int32_t w) { return w >= 2 ? 0xFFFFFFFFu / (uint32_t)w + 1u : 0u; }

// qr_replay_add (rule null) and qr_replay_add_rule: one set of checks, one argument block, two kernels
static int do_replay_add(const QrReplayAdd* r, const QrReplayAddRule* rule, void* stream) {
  if (!r) return QR_E_NULL;
  if (r->n_agents < 1 || r->n_agents > 2 || r->reserved0 != 0 || r->capacity < 1 || r->n_steps < 1 || r->n_envs < 1) return QR_E_SIZE;
  if (r->n_envs > r->capacity || (int64_t)r->n_steps * r->n_envs > r->capacity) return QR_E_SIZE;
  if (!r->state && (r->count < 0 || r->count >= r->capacity)) return QR_E_SIZE;
  if (r->action_row < 1) return QR_E_SIZE;
  for (int k = 0; k < r->n_agents; ++k) {
    if (r->obs_dim[k] < 1 || r->obs_dim[k] > kReplayMaxWidth || r->action_dim[k] < 1 || r->action_dim[k] > kReplayMaxWidth) return QR_E_SIZE;
    if (r->col_offset[k] < 0 || (int64_t)r->col_offset[k] + r->action_dim[k] > r->action_row) return QR_E_SIZE;
  }
  if (rule) {
    const auto finite_from = [](double v, bool zero) { return (zero ? v >= 0.0 : v > 0.0) && v <= 1.7e308; };   // (a NaN fails)
    if (!finite_from(rule->pos_tol, true) || !finite_from(rule->rot_tol, true) || !finite_from(rule->x_lim, false)) return QR_E_SIZE;
    if (r->obs_dim[0] < 3) return QR_E_SIZE;   // (agent 0's rule reads ex: three words)
  }
  if (!r->action || !r->reward || !r->done || (rule && !r->truncated)) return QR_E_NULL;
  for (int k = 0; k < r->n_agents; ++k)
    if (!r->obs[k] || !r->buf_obs[k] || !r->buf_obs_next[k] || !r->buf_action[k] || !r->buf_reward[k] || !r->buf_done[k]) return QR_E_NULL;
  if (r->n_agents == 2 && (r->final_obs[0] == nullptr) != (r->final_obs[1] == nullptr)) return QR_E_NULL;
  uintptr_t bits = reinterpret_cast<uintptr_t>(r->action) | reinterpret_cast<uintptr_t>(r->reward);
  for (int k = 0; k < r->n_agents; ++k)
    for (const void* p : {(const void*)r->obs[k], (const void*)r->final_obs[k], (const void*)r->buf_obs[k], (const void*)r->buf_obs_next[k],
                          (const void*)r->buf_action[k], (const void*)r->buf_reward[k], (const void*)r->buf_done[k]})
      bits |= reinterpret_cast<uintptr_t>(p);
  if ((bits & 3u) || (reinterpret_cast<uintptr_t>(r->state) & 7u)) return QR_E_ALIGN;
  const bool two = r->n_agents == 2;
  ReplayAddArgs a{};
  a.obs0 = r->obs[0]; a.final0 = r->final_obs[0];
  a.b_obs0 = r->buf_obs[0]; a.b_next0 = r->buf_obs_next[0]; a.b_act0 = r->buf_action[0]; a.b_rwd0 = r->buf_reward[0]; a.b_done0 = r->buf_done[0];
  a.D0 = r->obs_dim[0]; a.A0 = r->action_dim[0]; a.col0 = r->col_offset[0]; a.next0 = r->n_envs * r->obs_dim[0];
  a.mD0 = replay_magic(a.D0); a.mA0 = replay_magic(a.A0);
  if (two) {
    a.obs1 = r->obs[1]; a.final1 = r->final_obs[1];
    a.b_obs1 = r->buf_obs[1]; a.b_next1 = r->buf_obs_next[1]; a.b_act1 = r->buf_action[1]; a.b_rwd1 = r->buf_reward[1]; a.b_done1 = r->buf_done[1];
    a.D1 = r->obs_dim[1]; a.A1 = r->action_dim[1]; a.col1 = r->col_offset[1]; a.next1 = r->n_envs * r->obs_dim[1];
    a.mD1 = replay_magic(a.D1); a.mA1 = replay_magic(a.A1);
  }
  a.action = r->action; a.reward = r->reward; a.done = r->done; a.truncated = r->truncated;
  a.state = r->state; a.count = r->count; a.capacity = r->capacity; a.rows = (int64_t)r->n_steps * r->n_envs;
  a.action_row = r->action_row; a.n_agents = r->n_agents;
  const int64_t tiles = (a.rows + kReplayTile - 1) / kReplayTile;
  const dim3 grid((unsigned)(tiles < kReplayCols ? tiles : kReplayCols), (unsigned)(kReplaySegments * r->n_agents));
  if (rule) {
    const ReplayAddRuleArgs ra{a, ReplayRule{rule->x_lim, rule->pos_tol, rule->rot_tol}};
    hipLaunchKernelGGL(replay_add_rule_kernel, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), ra);
  } else {
    hipLaunchKernelGGL(replay_add_kernel, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  }
  if (int rc = (int)hipGetLastError()) return rc;
  if (r->state) hipLaunchKernelGGL(replay_advance_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), r->state, a.rows, r->capacity, (int64_t)0);
  return (int)hipGetLastError();
}

static int do_replay_sample(const QrReplaySample* s, void* stream) {
  if (!s) return QR_E_NULL;
  if (s->batch < 1 || s->batch > s->n || s->n > 0x7FFFFFFFll) return QR_E_SIZE;
  if (!s->index) return QR_E_NULL;
  if (((reinterpret_cast<uintptr_t>(s->index) | reinterpret_cast<uintptr_t>(s->state)) & 7u) || (reinterpret_cast<uintptr_t>(s->status) & 3u)) return QR_E_ALIGN;
  const ReplaySampleArgs a{s->index, s->status, s->state, s->n, s->batch, s->seed, s->draw};
  hipLaunchKernelGGL(replay_sample_kernel, dim3((unsigned)((s->batch + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  if (int rc = (int)hipGetLastError()) return rc;
  if (s->state) hipLaunchKernelGGL(replay_advance_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), s->state, (int64_t)0, (int64_t)1, (int64_t)1);
  return (int)hipGetLastError();
}

static int do_noise_fill(const QrNoiseFill* n, void* stream) {
  if (!n) return QR_E_NULL;
  if (n->n_slots < 1 || n->n_slots > kNoiseSlots) return QR_E_SIZE;
  int64_t quads = 0;
  for (int k = 0; k < n->n_slots; ++k) {
    const QrNoiseSlot& s = n->slot[k];
    if (s.count < 1 || s.count > 0x1FFFFFFFCll || s.kind > QR_NOISE_UNIFORM || s.stream >= (1u << 30)) return QR_E_SIZE;
    if (!__builtin_isfinite(s.a) || !__builtin_isfinite(s.b)) return QR_E_SIZE;
    quads += (s.count + 3) / 4;
  }
  if (quads > 0x7FFFFFFFll || (!n->draw_dev && n->draw < 0)) return QR_E_SIZE;
  for (int k = 0; k < n->n_slots; ++k)
    if (!n->slot[k].out) return QR_E_NULL;
  for (int k = 0; k < n->n_slots; ++k)
    if (reinterpret_cast<uintptr_t>(n->slot[k].out) & 3u) return QR_E_ALIGN;
  if (reinterpret_cast<uintptr_t>(n->draw_dev) & 7u) return QR_E_ALIGN;
  NoiseArgs a{};
  quads = 0;
  for (int k = 0; k < kNoiseSlots; ++k) {
    if (k < n->n_slots) {
      const QrNoiseSlot& s = n->slot[k];
      a.out[k] = s.out; a.count[k] = s.count; a.a[k] = s.a; a.b[k] = s.b; a.kind[k] = s.kind; a.stream[k] = s.stream;
      quads += (s.count + 3) / 4;
    }
    a.qend[k] = (uint32_t)quads;
  }
  a.seed = n->seed; a.draw_dev = n->draw_dev; a.draw = n->draw;
  const int64_t blocks = (quads + kNoiseBlock - 1) / kNoiseBlock;
  hipLaunchKernelGGL(noise_fill_kernel, dim3((unsigned)(blocks < kNoiseGrid ? blocks : kNoiseGrid)), dim3(kNoiseBlock), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  return (int)hipGetLastError();
}

static int do_shuffle(const QrShuffle* p, void* stream) {
  if (!p) return QR_E_NULL;
  if (p->n < 1 || p->n > 0xFFFFFFFFll || p->first < 0 || p->count < 0 || p->first > p->n || p->count > p->n - p->first) return QR_E_SIZE;
  if (p->stream >= (1u << 30) || p->max_workgroups < 0 || (!p->draw_dev && p->draw < 0)) return QR_E_SIZE;
  if (p->count == 0) return 0;
  if (!p->out) return QR_E_NULL;
  if ((reinterpret_cast<uintptr_t>(p->out) | reinterpret_cast<uintptr_t>(p->draw_dev)) & 7u) return QR_E_ALIGN;
  uint32_t w = 1;
  while (w < 16 && (1ull << (2 * w)) < (uint64_t)p->n) ++w;
  const ShuffleArgs a{p->out, p->draw_dev, p->draw, p->seed, (uint32_t)p->n, (uint32_t)p->first, (uint32_t)p->count, p->stream, w};
  const int64_t blocks = (p->count + kShuffleBlock - 1) / kShuffleBlock, cap = p->max_workgroups > 0 ? p->max_workgroups : kShuffleGrid;
  hipLaunchKernelGGL(shuffle_kernel, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(kShuffleBlock), 0, reinterpret_cast<hipStream_t>(stream), a);
  return (int)hipGetLastError();
}

static int do_episode_scan(const QrEpisodeScan* e, void* stream) {
  if (!e) return QR_E_NULL;
  const bool two = e->n_agents == 2;
  if (e->n_steps < 1 || e->n_envs < 0 || e->n_envs > (1ll << 36) || e->n_agents < 1 || e->n_agents > 2 || e->reserved0 != 0) return QR_E_SIZE;
  if (e->d0 < 3 || (two && e->d1 < 1)) return QR_E_SIZE;
  const auto finite_from = [](double v, bool zero) { return (zero ? v >= 0.0 : v > 0.0) && v <= 1.7e308; };   // (a NaN fails)
  if (!finite_from(e->pos_tol, true) || !finite_from(e->rot_tol, true) || !finite_from(e->x_lim, false)) return QR_E_SIZE;
  const int64_t tiles = e->n_envs > 0 ? (e->n_envs + 63) / 64 : 1;
  if (e->workspace_bytes < tiles * kEpK * (int64_t)sizeof(double)) return QR_E_SIZE;
  if (!e->reward || !e->done || !e->truncated || !e->run_return || !e->run_length || !e->last || !e->total || !e->workspace) return QR_E_NULL;
  if (e->final_obs0 ? (two && !e->final_obs1) : e->ep_final_error != nullptr) return QR_E_NULL;
  uintptr_t b4 = reinterpret_cast<uintptr_t>(e->reward) | reinterpret_cast<uintptr_t>(e->final_obs0) | reinterpret_cast<uintptr_t>(e->run_length) |
                 reinterpret_cast<uintptr_t>(e->ep_length);
  if (two && e->final_obs0) b4 |= reinterpret_cast<uintptr_t>(e->final_obs1);
  const uintptr_t b8 = reinterpret_cast<uintptr_t>(e->run_return) | reinterpret_cast<uintptr_t>(e->ep_return) | reinterpret_cast<uintptr_t>(e->last) |
                       reinterpret_cast<uintptr_t>(e->total) | reinterpret_cast<uintptr_t>(e->workspace) | (two ? reinterpret_cast<uintptr_t>(e->reward) : 0);
  if ((b4 & 3u) || (b8 & 7u) || (reinterpret_cast<uintptr_t>(e->ep_final_error) & 15u)) return QR_E_ALIGN;
  if (e->n_envs == 0) return 0;
  const EpisodeScanArgs a{e->reward, e->done, e->truncated, e->final_obs0, e->final_obs0 && two ? e->final_obs1 : nullptr, e->run_return, e->run_length,
                          e->ep_return, e->ep_length, e->ep_flags, e->ep_final_error, static_cast<double*>(e->workspace), e->n_envs, e->n_steps,
                          e->d0, two ? e->d1 : 0, e->record != 0 ? 1 : 0, e->x_lim, e->pos_tol, e->rot_tol};
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (two) hipLaunchKernelGGL(episode_scan_kernel<2>, dim3((unsigned)tiles), dim3(64), 0, s, a);
  else hipLaunchKernelGGL(episode_scan_kernel<1>, dim3((unsigned)tiles), dim3(64), 0, s, a);
  if (int rc = (int)hipGetLastError()) return rc;
  const EpisodeReduceArgs o{a.partials, e->last, e->total, (int32_t)tiles, e->n_steps, a.record};
  hipLaunchKernelGGL(episode_reduce_kernel, dim3(1), dim3(256), 0, s, o);
  return (int)hipGetLastError();
}

static int64_t gae_rule_tiles(int64_t n_envs, int32_t n_agents) {
  const int64_t m = n_envs * n_agents;
  return m > 0 ? (m + 63) / 64 : 1;
}

static int do_gae_rule(const QrGaeRule* e, void* stream) {
  if (!e) return QR_E_NULL;
  const bool two = e->n_agents == 2;
  if (e->n_steps < 1 || e->n_envs < 0 || e->n_envs > (1ll << 35) || e->n_agents < 1 || e->n_agents > 2 || e->reserved0 != 0) return QR_E_SIZE;
  if (e->rule < 0 || e->rule > 1) return QR_E_SIZE;
  const auto finite_from = [](double v, bool zero) { return (zero ? v >= 0.0 : v > 0.0) && v <= 1.7e308; };   // (a NaN fails)
  if (e->rule) {
    if (e->d0 < 3 || (two && e->d1 < 1)) return QR_E_SIZE;
    if (!finite_from(e->pos_tol, true) || !finite_from(e->rot_tol, true) || !finite_from(e->x_lim, false)) return QR_E_SIZE;
  }
  if (e->normalized && (!finite_from(e->norm_eps, true) || (int64_t)e->n_steps * e->n_envs < 2)) return QR_E_SIZE;
  const int64_t tiles = gae_rule_tiles(e->n_envs, e->n_agents);
  const int fields = 2 * e->n_agents;
  if (e->stats && e->workspace_bytes < tiles * fields * (int64_t)sizeof(double)) return QR_E_SIZE;
  if (!e->reward || !e->done || !e->value || !e->advantage || !e->td_target) return QR_E_NULL;
  if (e->rule && (!e->truncated || !e->term_obs0 || (two && !e->term_obs1))) return QR_E_NULL;
  if ((e->normalized && !e->stats) || (e->stats && !e->workspace)) return QR_E_NULL;
  uintptr_t b4 = reinterpret_cast<uintptr_t>(e->reward) | reinterpret_cast<uintptr_t>(e->value) | reinterpret_cast<uintptr_t>(e->next_value) |
                 reinterpret_cast<uintptr_t>(e->advantage) | reinterpret_cast<uintptr_t>(e->td_target) | reinterpret_cast<uintptr_t>(e->normalized);
  if (e->rule) b4 |= reinterpret_cast<uintptr_t>(e->term_obs0) | (two ? reinterpret_cast<uintptr_t>(e->term_obs1) : 0);
  uintptr_t b8 = reinterpret_cast<uintptr_t>(e->stats);
  if (e->stats) b8 |= reinterpret_cast<uintptr_t>(e->workspace);
  if ((b4 & 3u) || (b8 & 7u)) return QR_E_ALIGN;
  if (e->n_envs == 0) return 0;
  const GaeRuleArgs g{e->reward, e->done, e->rule ? e->truncated : nullptr, e->rule ? e->term_obs0 : nullptr, e->rule && two ? e->term_obs1 : nullptr,
                      e->value, e->next_value, e->advantage, e->td_target, e->done_eff, e->stats ? static_cast<double*>(e->workspace) : nullptr,
                      e->n_envs, e->n_steps, e->d0, two ? e->d1 : 0, e->rule, e->gamma, e->lam, e->x_lim, e->pos_tol, e->rot_tol};
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (two) hipLaunchKernelGGL(gae_rule_kernel<2>, dim3((unsigned)tiles), dim3(64), 0, s, g);
  else hipLaunchKernelGGL(gae_rule_kernel<1>, dim3((unsigned)tiles), dim3(64), 0, s, g);
  if (int rc = (int)hipGetLastError()) return rc;
  if (!e->stats) return 0;
  const GaeFoldArgs o{g.partials, e->stats, (int32_t)tiles, fields, (double)((int64_t)e->n_steps * e->n_envs)};
  hipLaunchKernelGGL(gae_fold_kernel, dim3(1), dim3(256), 0, s, o);
  if (int rc = (int)hipGetLastError()) return rc;
  if (!e->normalized) return 0;
  const GaeNormArgs q{e->advantage, e->stats, e->normalized, (int64_t)e->n_steps * e->n_envs * e->n_agents, e->norm_eps};
  const bool vec = ((reinterpret_cast<uintptr_t>(e->advantage) | reinterpret_cast<uintptr_t>(e->normalized)) & 15u) == 0;
  const int64_t per = vec ? 1024 : 256;   // elements a workgroup takes per sweep
  const int64_t blocks = (q.count + per - 1) / per;
  const dim3 grid((unsigned)(blocks < kGaeNormGrid ? blocks : kGaeNormGrid));
  if (two) {
    if (vec) hipLaunchKernelGGL((gae_normalize_kernel<2, true>), grid, dim3(256), 0, s, q);
    else hipLaunchKernelGGL((gae_normalize_kernel<2, false>), grid, dim3(256), 0, s, q);
  } else {
    if (vec) hipLaunchKernelGGL((gae_normalize_kernel<1, true>), grid, dim3(256), 0, s, q);
    else hipLaunchKernelGGL((gae_normalize_kernel<1, false>), grid, dim3(256), 0, s, q);
  }
  return (int)hipGetLastError();
}

// What qr_es_perturb and qr_es_gradient check alike in their sizes: P, the tensors' counts and stream ids, sigma, the grid cap and the
// generation.  quads: the sum of ceil(count / 4) over the tensors.
static int es_sizes(const QrEsTensor* t, int32_t n_tensors, int32_t P, float sigma, float reserved0, int32_t max_workgroups,
                    const int64_t* generation_dev, int64_t generation, int64_t* quads) {
  if (P < 2 || (P & 1) || P > QR_ES_MAX_POLICIES || n_tensors < 1 || n_tensors > kEsSlots) return QR_E_SIZE;
  *quads = 0;
  for (int k = 0; k < n_tensors; ++k) {
    if (t[k].count < 1 || t[k].count > 0x7FFFFFFFll || t[k].stream >= (1u << 30) || t[k].reserved0 != 0) return QR_E_SIZE;
    for (int m = 0; m < k; ++m)
      if (t[m].stream == t[k].stream) return QR_E_SIZE;
    *quads += (t[k].count + 3) / 4;
  }
  if (*quads * (P / 2) > 0x7FFFFFFFll) return QR_E_SIZE;
  if (!(sigma > 0.0f) || !__builtin_isfinite(sigma) || reserved0 != 0.0f || max_workgroups < 0) return QR_E_SIZE;
  if (!generation_dev && generation < 0) return QR_E_SIZE;
  return 0;
}

static int do_es_perturb(const QrEsPerturb* p, void* stream) {
  if (!p) return QR_E_NULL;
  int64_t quads = 0;
  if (int rc = es_sizes(p->tensor, p->n_tensors, p->n_policies, p->sigma, p->reserved0, p->max_workgroups, p->generation_dev, p->generation, &quads))
    return rc;
  if (p->n_copies < 0 || p->n_copies > kEsCopies) return QR_E_SIZE;
  for (int c = 0; c < p->n_copies; ++c)
    if (p->copy[c].count < 1 || p->copy[c].count > 0x7FFFFFFFll) return QR_E_SIZE;
  uintptr_t b4 = 0;
  for (int k = 0; k < p->n_tensors; ++k) {
    if (!p->tensor[k].base || !p->tensor[k].out) return QR_E_NULL;
    b4 |= reinterpret_cast<uintptr_t>(p->tensor[k].base) | reinterpret_cast<uintptr_t>(p->tensor[k].out);
  }
  for (int c = 0; c < p->n_copies; ++c) {
    if (!p->copy[c].src || !p->copy[c].dst) return QR_E_NULL;
    b4 |= reinterpret_cast<uintptr_t>(p->copy[c].src) | reinterpret_cast<uintptr_t>(p->copy[c].dst);
  }
  if ((b4 & 3u) || (reinterpret_cast<uintptr_t>(p->generation_dev) & 7u)) return QR_E_ALIGN;
  EsPerturbArgs a{};
  const int64_t half = p->n_policies / 2;
  int64_t end = 0;
  for (int k = 0; k < kEsSlots; ++k) {
    if (k < p->n_tensors) {
      const QrEsTensor& t = p->tensor[k];
      a.base[k] = t.base; a.out[k] = t.out; a.count[k] = (uint32_t)t.count; a.quads[k] = (uint32_t)((t.count + 3) / 4); a.stream[k] = t.stream;
      end += half * a.quads[k];
    }
    a.qend[k] = (uint32_t)end;
  }
  for (int c = 0; c < p->n_copies; ++c) { a.csrc[c] = p->copy[c].src; a.cdst[c] = p->copy[c].dst; a.ccount[c] = (uint32_t)p->copy[c].count; }
  a.n_copies = p->n_copies; a.P = (uint32_t)p->n_policies; a.sigma = p->sigma;
  a.seed = p->seed; a.gen_dev = p->generation_dev; a.gen = p->generation;
  const int64_t blocks = (end + kEsBlock - 1) / kEsBlock, cap = p->max_workgroups > 0 && p->max_workgroups < kEsGrid ? p->max_workgroups : kEsGrid;
  hipLaunchKernelGGL(es_perturb_kernel, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(kEsBlock), 0, reinterpret_cast<hipStream_t>(stream), a);
  return (int)hipGetLastError();
}

static int do_es_gradient(const QrEsGradient* g, void* stream) {
  if (!g) return QR_E_NULL;
  int64_t quads = 0;
  if (int rc = es_sizes(g->tensor, g->n_tensors, g->n_policies, g->sigma, g->reserved0, g->max_workgroups, g->generation_dev, g->generation, &quads))
    return rc;
  if (g->shaping < QR_ES_CENTERED_RANK || g->shaping > QR_ES_STANDARDIZE) return QR_E_SIZE;
  if (g->workspace_bytes < (int64_t)(g->n_policies / 2) * (int64_t)sizeof(double)) return QR_E_SIZE;
  uintptr_t b4 = reinterpret_cast<uintptr_t>(g->fitness);
  for (int k = 0; k < g->n_tensors; ++k) {
    if (!g->tensor[k].out) return QR_E_NULL;
    b4 |= reinterpret_cast<uintptr_t>(g->tensor[k].out);
  }
  if (!g->fitness || !g->stats || !g->workspace) return QR_E_NULL;
  const uintptr_t b8 = reinterpret_cast<uintptr_t>(g->stats) | reinterpret_cast<uintptr_t>(g->workspace) | reinterpret_cast<uintptr_t>(g->generation_dev);
  if ((b4 & 3u) || (b8 & 7u)) return QR_E_ALIGN;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const EsUtilityArgs u{g->fitness, static_cast<double*>(g->workspace), g->stats, g->n_policies, g->shaping};
  hipLaunchKernelGGL(es_utility_kernel, dim3((unsigned)((g->n_policies + kEsBlock - 1) / kEsBlock)), dim3(kEsBlock), 0, s, u);
  if (int rc = (int)hipGetLastError()) return rc;
  EsGradArgs a{};
  int64_t end = 0;
  for (int k = 0; k < kEsSlots; ++k) {
    if (k < g->n_tensors) {
      const QrEsTensor& t = g->tensor[k];
      a.grad[k] = t.out; a.count[k] = (uint32_t)t.count; a.quads[k] = (uint32_t)((t.count + 3) / 4); a.stream[k] = t.stream;
      end += a.quads[k];
    }
    a.qend[k] = (uint32_t)end;
  }
  a.w = u.w; a.half = (uint32_t)(g->n_policies / 2); a.den = (double)g->n_policies * (double)g->sigma;
  a.seed = g->seed; a.gen_dev = g->generation_dev; a.gen = g->generation;
  const int64_t cap = g->max_workgroups > 0 && g->max_workgroups < kEsGradGrid ? g->max_workgroups : kEsGradGrid;
  hipLaunchKernelGGL(es_grad_kernel, dim3((unsigned)(end < cap ? end : cap)), dim3(64), 0, s, a);
  return (int)hipGetLastError();
}
}  // namespace qr

extern "C" {

int qr_es_perturb(const QrEsPerturb* p, void* stream) { return qr::do_es_perturb(p, stream); }

int qr_es_gradient(const QrEsGradient* g, void* stream) { return qr::do_es_gradient(g, stream); }

int64_t qr_es_workspace_bytes(int32_t n_policies) {
  if (n_policies < 2 || (n_policies & 1) || n_policies > QR_ES_MAX_POLICIES) return QR_E_SIZE;
  return (int64_t)(n_policies / 2) * (int64_t)sizeof(double);
}

int qr_gae_rule(const QrGaeRule* a, void* stream) { return qr::do_gae_rule(a, stream); }

int64_t qr_gae_rule_workspace_bytes(int64_t n_envs, int32_t n_agents) {
  if (n_envs < 0 || n_agents < 1 || n_agents > 2) return QR_E_SIZE;
  return qr::gae_rule_tiles(n_envs, n_agents) * 2 * n_agents * (int64_t)sizeof(double);
}

int qr_episode_scan(const QrEpisodeScan* a, void* stream) { return qr::do_episode_scan(a, stream); }

int64_t qr_episode_workspace_bytes(int64_t n_envs) {
  if (n_envs < 0) return QR_E_SIZE;
  return (n_envs > 0 ? (n_envs + 63) / 64 : 1) * qr::kEpK * (int64_t)sizeof(double);
}

int qr_noise_fill(const QrNoiseFill* fill, void* stream) { return qr::do_noise_fill(fill, stream); }
int qr_shuffle(const QrShuffle* shuffle, void* stream) { return qr::do_shuffle(shuffle, stream); }

int qr_replay_add(const QrReplayAdd* add, void* stream) { return qr::do_replay_add(add, nullptr, stream); }

int qr_replay_add_rule(const QrReplayAddRule* rule, void* stream) {
  return rule ? qr::do_replay_add(&rule->add, rule, stream) : QR_E_NULL;
}

int qr_replay_sample(const QrReplaySample* sample, void* stream) { return qr::do_replay_sample(sample, stream); }

int qr_dpg_actor_grad(const QrActor* actor, const QrQCritic* critic, const QrTransitions* batch, const QrDpgGrad* grad, void* stream) {
  return qr::do_dpg_actor(actor, critic, batch, grad, stream);
}

int64_t qr_dpg_actor_workspace_bytes(int32_t obs_dim, int32_t hidden_dim, int32_t action_dim, int32_t critic_hidden_dim, int64_t batch,
                                     int32_t max_workgroups) {
  const int size = qr::actor_size(obs_dim, hidden_dim, action_dim);
  if (size < 0 || critic_hidden_dim < 1 || critic_hidden_dim > 64 || batch < 1 || max_workgroups < 0) return QR_E_SIZE;
  return qr::ppo_grid(batch, max_workgroups) * qr::kDpgNP[size] * (int64_t)sizeof(double);
}

int qr_ctde_dpg_actor_grad(const QrActor* actor_0, const QrActor* actor_1, const QrQCritic* critic, const QrCtdeTransitions* batch,
                           const QrCtdeDpgGrad* grad, void* stream) {
  return qr::do_ctde_dpg_actor(actor_0, actor_1, critic, batch, grad, stream);
}

int64_t qr_ctde_dpg_actor_workspace_bytes(int32_t agent, int32_t critic_hidden_dim, int64_t batch, int32_t max_workgroups) {
  if ((agent != 0 && agent != 1) || critic_hidden_dim < 1 || critic_hidden_dim > 64 || batch < 1 || max_workgroups < 0) return QR_E_SIZE;
  return qr::ppo_grid(batch, max_workgroups) * qr::kDpgNP[1 + agent] * (int64_t)sizeof(double);
}

int qr_soft_update(const QrSoftUpdate* update, void* stream) { return qr::do_soft_update(update, stream); }

int qr_sac_target(const QrActor* actor, const QrQCritic* critic_target, const QrTransitions* batch, const QrSacTarget* target, void* stream) {
  return qr::do_sac_target(actor, critic_target, batch, target, stream);
}

int qr_sac_actor_grad(const QrActor* actor, const QrQCritic* critic, const QrTransitions* batch, const QrSacActorGrad* grad, void* stream) {
  return qr::do_sac_actor(actor, critic, batch, grad, stream);
}

int64_t qr_sac_actor_workspace_bytes(int32_t obs_dim, int32_t hidden_dim, int32_t action_dim, int32_t critic_hidden_dim, int64_t batch,
                                     int32_t max_workgroups) {
  const int size = qr::actor_size(obs_dim, hidden_dim, action_dim);
  if (size < 0 || critic_hidden_dim < 1 || critic_hidden_dim > 64 || batch < 1 || max_workgroups < 0) return QR_E_SIZE;
  return qr::ppo_grid(batch, max_workgroups) * qr::kSacNP[size] * (int64_t)sizeof(double);
}

int qr_ctde_sac_actor_grad(const QrActor* actor_0, const QrActor* actor_1, const QrQCritic* critic, const QrCtdeTransitions* batch,
                           const QrCtdeSacActorGrad* grad, void* stream) {
  return qr::do_ctde_sac_actor(actor_0, actor_1, critic, batch, grad, stream);
}

int64_t qr_ctde_sac_actor_workspace_bytes(int32_t agent, int32_t critic_hidden_dim, int64_t batch, int32_t max_workgroups) {
  if ((agent != 0 && agent != 1) || critic_hidden_dim < 1 || critic_hidden_dim > 64 || batch < 1 || max_workgroups < 0) return QR_E_SIZE;
  return qr::ppo_grid(batch, max_workgroups) * qr::kSacNP[1 + agent] * (int64_t)sizeof(double);
}

int qr_twinq_target(const QrActor* actor_target, const QrQCritic* critic_target, const QrTransitions* batch, const QrTd3Target* target,
                  void* stream) {
  return qr::do_td3_target(actor_target, critic_target, batch, target, stream);
}

int qr_twinq_grad(const QrQCritic* critic, const QrTransitions* batch, const QrTwinQGrad* grad, void* stream) {
  return qr::do_twinq(critic, batch, grad, stream);
}

int qr_ctde_twinq_target(const QrActor* actor_target_0, const QrActor* actor_target_1, const QrQCritic* critic_target,
                         const QrCtdeTransitions* batch, const QrCtdeTd3Target* target, void* stream) {
  return qr::do_ctde_td3_target(actor_target_0, actor_target_1, critic_target, batch, target, stream);
}

int qr_ctde_sac_target(const QrActor* actor_0, const QrActor* actor_1, const QrQCritic* critic_target, const QrCtdeTransitions* batch,
                       const QrCtdeSacTarget* target, void* stream) {
  return qr::do_ctde_sac_target(actor_0, actor_1, critic_target, batch, target, stream);
}

int qr_ctde_twinq_grad(const QrQCritic* critic, const QrCtdeTransitions* batch, const QrTwinQGrad* grad, void* stream) {
  return qr::do_ctde_twinq(critic, batch, grad, stream);
}

int64_t qr_ctde_twinq_workspace_bytes(int32_t in_dim, int32_t hidden_dim, int64_t batch, int32_t max_workgroups) {
  if (in_dim < 4) return QR_E_SIZE;
  return qr_twinq_workspace_bytes(in_dim, hidden_dim, batch, max_workgroups);
}

int64_t qr_twinq_workspace_bytes(int32_t in_dim, int32_t hidden_dim, int64_t batch, int32_t max_workgroups) {
  if (in_dim < 2 || !qr::twinq_sizes_ok(in_dim - 1, 1, hidden_dim) || batch < 1 || max_workgroups < 0) return QR_E_SIZE;
  return 2 * qr::twinq_grid(batch, max_workgroups) * qr::MlpGradLayout(in_dim, hidden_dim, qr::kTqSums).np * (int64_t)sizeof(double);
}

int qr_adamw_step(const QrAdamWGroup* groups, int32_t n_groups, void* stream) { return qr::do_adamw(groups, n_groups, stream); }

int qr_adamw_polyak_step(const QrAdamWPolyakGroup* groups, int32_t n_groups, void* stream) {
  return qr::do_adamw_polyak(groups, n_groups, stream);
}

int qr_ppo_critic_grad(const QrCritic* critic, const QrCriticBatch* batch, const QrCriticGrad* grad, void* stream) {
  return qr::do_ppo_critic(critic, batch, grad, stream);
}

int64_t qr_ppo_critic_workspace_bytes(int32_t in_dim, int32_t hidden_dim, int64_t batch, int32_t max_workgroups) {
  if (!qr::ppo_critic_sizes_ok(in_dim, 0, hidden_dim) || batch < 1 || max_workgroups < 0) return QR_E_SIZE;
  return qr::ppo_critic_grid(batch, max_workgroups) * qr::MlpGradLayout(in_dim, hidden_dim, qr::kPcSums).np * (int64_t)sizeof(double);
}

int qr_ppo_actor_grad(const QrActor* actor, const QrPpoBatch* batch, const QrPpoGrad* grad, void* stream) {
  return qr::do_ppo_actor(actor, batch, grad, nullptr, stream);
}
int qr_ppo_actor_grad_dev(const QrActor* actor, const QrPpoBatch* batch, const QrPpoGrad* grad, const float* entropy_coef_dev, void* stream) {
  return qr::do_ppo_actor(actor, batch, grad, entropy_coef_dev, stream);
}

int64_t qr_ppo_actor_workspace_bytes(int32_t obs_dim, int32_t hidden_dim, int32_t action_dim, int64_t batch, int32_t max_workgroups) {
  const int size = qr::actor_size(obs_dim, hidden_dim, action_dim);
  if (size < 0 || batch < 1 || max_workgroups < 0) return QR_E_SIZE;
  return qr::ppo_grid(batch, max_workgroups) * qr::kPpoNP[size] * (int64_t)sizeof(double);
}

int qr_critic_values(const QrCritic* critic, const float* obs0, const float* obs1, int64_t n_rows, float* value, int32_t value_stride,
                     void* stream) {
  return qr::do_critic(critic, obs0, obs1, nullptr, 0, nullptr, n_rows, 0, nullptr, value, value_stride, false, stream);
}

int qr_critic_next_values(const QrCritic* critic, const float* final_obs0, const float* final_obs1, const uint8_t* done, int32_t n_agents,
                          const uint8_t* truncated, int32_t n_steps, int64_t n_envs, const float* value, float* next_value,
                          int32_t value_stride, void* stream) {
  if (!critic) return QR_E_NULL;
  if (n_steps < 1) return QR_E_SIZE;
  return qr::do_critic(critic, final_obs0, final_obs1, done, n_agents, truncated, n_envs < 0 ? n_envs : (int64_t)n_steps * n_envs, n_envs, value,
                       next_value, value_stride, true, stream);
}

#ifdef QR_SPAN
int qr_debug_set_span(void* buf) {  // diagnostic build only: device buffer [slots][2 * tiles][2] of uint64 (NULL = off) for the NEXT launches
  qr::g_span_buf = reinterpret_cast<unsigned long long*>(buf);
  return 0;
}
void qr_debug_set_span_slot(int slot) { qr::g_span_slot = slot; }  // the row the NEXT launches write (baked into a captured launch)
#endif

int qr_abi_version(void) { return QR_ABI_VERSION; }

void qr_default_coeffs(QrCoeffs* c) {
  if (!c) return;
  c->Cx = 6.0; c->CIx = 0.1; c->Cv = 0.4; c->Cb1 = 6.0; c->CIb1 = 0.1; c->CW = 0.6;  // args_parse.py:23-31, quad.py:80
  c->Cw12 = 0.6; c->CW3 = 0.1; c->alpha = 0.01; c->beta = 0.05;
  c->dt = 1.0 / 200.0;
  c->x_lim = 1.0; c->v_lim = 4.0; c->W_lim = 2.0 * qr::kPi;
  c->eIx_lim = 3.0; c->eIb1_lim = 3.0; c->euler_lim_deg = 85.0; c->udm_fraction = 0.1;
  c->eight_T = 9.0; c->eight_A1 = 1.5; c->eight_A2 = 1.0; c->eight_w_b1d = 0.349066; c->eight_alt_d = -0.6;  // trajectory_generator.py:98-110
  c->eight_eps = 0.01; c->eight_count = 3.0;
  c->w_adapt = 16.0;
  c->m_nominal = 2.15; c->d_nominal = 0.23; c->J1_nominal = 0.022; c->J3_nominal = 0.035;  // quad.py:28-33
  c->c_tf_nominal = 0.0135; c->c_tw_nominal = 2.2; c->g = 9.81; c->min_force = 0.5;         // quad.py:31-36
}

int qr_step(const QrEnv* env, const float* action, int32_t substeps, const QrStepOut* out, void* stream) {
  return qr::do_rollout(env, action, nullptr, 1, substeps, out, stream);
}

int qr_rollout(const QrEnv* env, const float* action, int32_t n_steps, int32_t substeps, const QrStepOut* out, void* stream) {
  return qr::do_rollout(env, action, nullptr, n_steps, substeps, out, stream);
}

int qr_rollout_actor(const QrEnv* env, const QrPolicyRollout* policy, int32_t n_steps, int32_t substeps, const QrStepOut* out,
                     void* stream) {
  if (!policy) return QR_E_NULL;
  return qr::do_rollout(env, nullptr, policy, n_steps, substeps, out, stream);
}

int qr_evaluate_actor(const QrEnv* env, const QrPolicyRollout* policy, int32_t max_steps, int32_t substeps, const QrEvalOut* out,
                      void* stream) {
  return qr::do_evaluate(env, policy, nullptr, max_steps, substeps, out, stream);
}

int qr_evaluate_population(const QrEnv* env, const QrPolicyRollout* policy, const QrPopulation* pop, int32_t max_steps,
                           int32_t substeps, const QrEvalOut* out, void* stream) {
  if (!pop) return QR_E_NULL;
  return qr::do_evaluate(env, policy, pop, max_steps, substeps, out, stream);
}

int qr_error_obs_format(const QrEnv* env, int32_t format, float* obs0, float* obs1, void* stream) {
  qr::Args a{};
  if (int rc = qr::fill_env(a, env)) return rc;
  if (env->kind == QR_KIND_QUAD) return QR_E_KIND;
  if (format != QR_KIND_COUPLED && format != QR_KIND_DECOUPLED) return QR_E_KIND;
  if (!env->integ || !obs0 || (format == QR_KIND_DECOUPLED && !obs1)) return QR_E_NULL;
  a.obs0 = obs0; a.obs1 = obs1;
  return qr::launch_tiles(a, env->layout, stream, [&](auto xv, auto qw, dim3 grid, hipStream_t s) {
    using XV = decltype(xv); using QW = decltype(qw);
    if (format == QR_KIND_COUPLED) hipLaunchKernelGGL((qr::error_obs_kernel<QR_KIND_COUPLED, XV, QW>), grid, dim3(64), 0, s, a);
    else hipLaunchKernelGGL((qr::error_obs_kernel<QR_KIND_DECOUPLED, XV, QW>), grid, dim3(64), 0, s, a);
  });
}

int qr_error_obs(const QrEnv* env, float* obs0, float* obs1, void* stream) {
  if (!env) return QR_E_NULL;
  return qr_error_obs_format(env, env->kind, obs0, obs1, stream);
}

int qr_reset(const QrEnv* env, const uint8_t* mask, void* stream) {
  qr::Args a{};
  if (int rc = qr::fill_env(a, env)) return rc;
  if (!env->episode) return QR_E_NULL;
  a.mask = mask;
  return qr::launch_tiles(a, env->layout, stream, [&](auto xv, auto qw, dim3 grid, hipStream_t s) {
    hipLaunchKernelGGL((qr::reset_kernel<decltype(xv), decltype(qw)>), grid, dim3(64), 0, s, a);
  });
}

int qr_get_state(const QrEnv* env, double* rows, void* stream) {
  qr::Args a{};
  if (int rc = qr::fill_env(a, env)) return rc;
  if (!rows) return QR_E_NULL;
  a.rows_out = rows;
  return qr::launch_tiles(a, env->layout, stream, [&](auto xv, auto qw, dim3 grid, hipStream_t s) {
    hipLaunchKernelGGL((qr::get_state_kernel<decltype(xv), decltype(qw)>), grid, dim3(64), 0, s, a);
  });
}

int qr_set_state(const QrEnv* env, const double* rows, const uint8_t* mask, int32_t* rejected, void* stream) {
  qr::Args a{};
  if (int rc = qr::fill_env(a, env)) return rc;
  if (!rows) return QR_E_NULL;
  a.rows_in = rows; a.mask = mask; a.status = rejected;
  return qr::launch_tiles(a, env->layout, stream, [&](auto xv, auto qw, dim3 grid, hipStream_t s) {
    hipLaunchKernelGGL((qr::set_state_kernel<decltype(xv), decltype(qw)>), grid, dim3(64), 0, s, a);
  });
}

int qr_check_state(const QrEnv* env, const double* rows, const uint8_t* mask, int32_t* rejected, void* stream) {
  qr::Args a{};
  if (int rc = qr::fill_env(a, env)) return rc;
  if (!rows || !rejected) return QR_E_NULL;
  a.rows_in = rows; a.mask = mask; a.status = rejected;
  a.dry_run = 1;  // count, write nothing
  return qr::launch_tiles(a, env->layout, stream, [&](auto xv, auto qw, dim3 grid, hipStream_t s) {
    hipLaunchKernelGGL((qr::set_state_kernel<decltype(xv), decltype(qw)>), grid, dim3(64), 0, s, a);
  });
}

int qr_traj_start(const QrEnv* env, const uint8_t* mask, const float* draws, void* stream) {
  qr::Args a{};
  if (int rc = qr::fill_env(a, env)) return rc;
  if (env->goal_mode == QR_GOAL_EXTERNAL) return QR_E_KIND;
  if (!draws && !env->episode) return QR_E_NULL;
  a.mask = mask; a.draws = draws;
  return qr::launch_tiles(a, env->layout, stream, [&](auto xv, auto qw, dim3 grid, hipStream_t s) {
    hipLaunchKernelGGL((qr::traj_start_kernel<decltype(xv), decltype(qw)>), grid, dim3(64), 0, s, a);
  });
}

int qr_get_desired(const QrEnv* env, const uint8_t* mask, float* rows, int32_t store_goal, void* stream) {
  qr::Args a{};
  if (int rc = qr::fill_env(a, env)) return rc;
  if (env->goal_mode == QR_GOAL_EXTERNAL) return QR_E_KIND;
  if (!rows && !store_goal) return QR_E_NULL;
  if (store_goal && !env->goal) return QR_E_NULL;
  a.goal_rows = rows; a.store_goal = store_goal; a.mask = mask;
  return qr::launch_tiles(a, env->layout, stream, [&](auto xv, auto qw, dim3 grid, hipStream_t s) {
    hipLaunchKernelGGL((qr::get_desired_kernel<decltype(xv), decltype(qw)>), grid, dim3(64), 0, s, a);
  });
}

int qr_gae(const float* reward, const uint8_t* done, const float* value, const float* next_value, int32_t n_steps,
           int64_t n_cols, float gamma, float lam, float* advantage, float* td_target, double* partials, void* stream) {
  if (!reward || !done || !value || !advantage || !td_target) return QR_E_NULL;
  if (n_steps < 1 || n_cols < 0) return QR_E_SIZE;
  if (n_cols == 0) return 0;
  qr::GaeArgs g{reward, done, value, next_value, advantage, td_target, partials, n_cols, n_steps, gamma, lam};
  hipLaunchKernelGGL(qr::gae_kernel, dim3((unsigned)((n_cols + 63) / 64)), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), g);
  return (int)hipGetLastError();
}

void qr_launch_thresholds(int32_t* step_quad, int32_t* step_wrappers, int32_t* rollout) {
  const qr::Tuning& tn = qr::tuning();
  if (step_quad) *step_quad = (int32_t)tn.helper_grid;
  if (step_wrappers) *step_wrappers = (int32_t)tn.helper_grid_wrap;
  if (rollout) *rollout = (int32_t)tn.helper_grid_rollout;
}

int qr_launch_plan(const QrEnv* env, int32_t n_steps, int32_t substeps, int32_t actor, QrLaunchPlan* plan) {
  if (!plan) return QR_E_NULL;
  memset(plan, 0, sizeof(*plan));
  qr::Args a{};
  if (int rc = qr::fill_env(a, env)) return rc;
  if (n_steps < 1 || substeps < 1 || actor < 0 || actor > 2) return QR_E_SIZE;
  if (actor && env->kind == QR_KIND_QUAD) return QR_E_KIND;
  a.n_steps = n_steps; a.substeps = substeps;
  if (actor) {  // qr_rollout_actor: what the decision reads of the policy block
    static float dummy;
    a.act_out = &dummy;
    a.actor[0].squash = a.actor[1].squash = actor == 2 ? QR_ACTOR_TANH_SAMPLE : QR_ACTOR_TANH_MEAN;
  }
  const unsigned tiles = (unsigned)((a.n + 63) / 64);
  const unsigned chunk = env->layout == QR_LAYOUT_MIXED ? qr::rollout_chunk(a, env->kind, env->layout) : 0u;
  const qr::Pick p = qr::pick_instance(a, env->kind, env->layout, chunk);
  plan->grid = (int32_t)(chunk ? chunk : tiles);
  plan->block = p.help ? 128 : 64;
  plan->launches = chunk ? (int32_t)((tiles + chunk - 1) / chunk) : 1;
  plan->traj = p.traj; plan->adapt = p.adapt; plan->policy = p.policy; plan->single = p.single; plan->help = p.help; plan->hrew = p.hrew;
  plan->mag = p.mag;
  plan->key = ((uint32_t)env->layout << 16) | ((uint32_t)env->kind << 8) | p.bits();
  static const char* const kXV[3] = {"float", "double", "float"};
  static const char* const kQW[3] = {"double", "double", "float"};
  snprintf(plan->name, sizeof(plan->name), "qr::step_kernel<%d,%s,%s,64,%d,%d,%d,%d,%d,%d,%d>", (int)env->kind, kXV[env->layout], kQW[env->layout],
           p.traj, (int)p.adapt, p.policy, (int)p.single, (int)p.help, (int)p.hrew, (int)p.mag);
  return 0;
}

const char* qr_step_kernel_info(const QrEnv* env, int32_t n_steps, int32_t* grid, int32_t* block) {
  QrLaunchPlan plan;
  if (qr_launch_plan(env, n_steps < 1 ? 1 : n_steps, 1, 0, &plan) != 0) return "";
  if (grid) *grid = plan.grid;
  if (block) *block = plan.block;
  switch (env->kind) {
    case QR_KIND_QUAD: return "qr::step_kernel<0,...>";
    case QR_KIND_COUPLED: return "qr::step_kernel<1,...>";
    case QR_KIND_DECOUPLED: return "qr::step_kernel<2,...>";
    default: return "";
  }
}

int32_t qr_launch_stats(uint32_t* keys, uint32_t* counts, int32_t capacity, int32_t reset) {
  int32_t n = 0;
  for (int l = 0; l < 3; ++l)
    for (int k = 0; k < 3; ++k)
      for (int b = 0; b < 512; ++b) {
        const uint32_t c = reset ? qr::g_launches[l][k][b].exchange(0u, std::memory_order_relaxed) : qr::g_launches[l][k][b].load(std::memory_order_relaxed);
        if (c == 0) continue;
        if (n < capacity && keys && counts) { keys[n] = ((uint32_t)l << 16) | ((uint32_t)k << 8) | (uint32_t)(b & 0xFF) | (b & 0x100 ? 0x1000u : 0u); counts[n] = c; }
        ++n;
      }
  return n;
}

int32_t qr_instance_table(uint32_t* keys, int32_t capacity) {
  int32_t n = 0;
  for (int l = 0; l < 3; ++l)
    for (int k = 0; k < 3; ++k) {
#define QR_X1(TR, AD, PO, SI, HE, HR, MG)                                                              \
  if (qr::inst_exists(k, l == QR_LAYOUT_MIXED, TR, AD, PO, SI, HE, HR, MG)) {                          \
    if (n < capacity && keys) keys[n] = ((uint32_t)l << 16) | ((uint32_t)k << 8) | qr::Pick{TR, (bool)AD, PO, (bool)SI, (bool)HE, (bool)HR, (bool)MG}.bits(); \
    ++n;                                                                                               \
  }
      QR_INSTANCES(QR_X)
#undef QR_X1
    }
  return n;
}

int qr_touch(const QrEnv* env, const float* action, const QrStepOut* out, void* stream) {
  qr::Args a{};
  if (int rc = qr::fill_env(a, env)) return rc;
  if (!action || !out || !out->reward || !out->done) return QR_E_NULL;
  if (env->kind != QR_KIND_QUAD && (!env->integ || !out->obs0)) return QR_E_NULL;
  if (env->kind == QR_KIND_DECOUPLED && !out->obs1) return QR_E_NULL;
  if (reinterpret_cast<uintptr_t>(action) & (env->kind == QR_KIND_DECOUPLED ? 3u : 15u)) return QR_E_ALIGN;
  a.action = action; a.obs0 = out->obs0; a.obs1 = out->obs1; a.reward = out->reward; a.done = out->done;
#ifdef QR_ONLY_KIND
  if (env->kind != QR_ONLY_KIND) return QR_E_KIND;
#endif
  return qr::launch_tiles(a, env->layout, stream, [&](auto xv, auto qw, dim3 grid, hipStream_t s) {
    using XV = decltype(xv); using QW = decltype(qw);
#define QR_TOUCH(KIND) hipLaunchKernelGGL((qr::touch_kernel<KIND, XV, QW>), grid, dim3(64), 0, s, a.pos_vel, a.att_rate, a.action, a.params, a.integ, a.reward, (int32_t)a.n, (int32_t)a.ld, a)
#ifdef QR_ONLY_KIND
    QR_TOUCH(QR_ONLY_KIND);
#else
    if (env->kind == QR_KIND_QUAD) QR_TOUCH(QR_KIND_QUAD);
    else if (env->kind == QR_KIND_COUPLED) QR_TOUCH(QR_KIND_COUPLED);
    else QR_TOUCH(QR_KIND_DECOUPLED);
#endif
#undef QR_TOUCH
  });
}

}  // extern "C"
