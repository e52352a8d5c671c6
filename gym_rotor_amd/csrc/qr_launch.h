// qr_launch.h — part of the gfx950 quadrotor step library (included by quadrotor_kernels.hip, in this order).
// Host side: argument blocks from the C structs, the launch rule, the instantiation table, launchers.
#pragma once
#include <stdlib.h>
#include <atomic>
#include "qr_step.h"
#include "qr_eval.h"
#include "qr_aux.h"

namespace qr {

// ------------------------------------------------------------------------------------
// Host side
// ------------------------------------------------------------------------------------
static float round_up_to_float(double v) {  // smallest float >= v
  float f = (float)v;
  if ((double)f < v) f = nextafterf(f, INFINITY);
  return f;
}

static void fill_coeffs(Coeffs& o, const QrCoeffs& q) {
  o.Cx = (float)q.Cx; o.CIx = (float)q.CIx; o.Cv = (float)q.Cv; o.Cb1 = (float)q.Cb1; o.CIb1 = (float)q.CIb1; o.CW = (float)q.CW;
  o.Cw12 = (float)q.Cw12; o.CW3 = (float)q.CW3;
  o.alpha = (float)q.alpha; o.beta = (float)q.beta; o.dt = q.dt; o.hdt = (float)(q.dt * 0.5);
  o.x_lim = q.x_lim; o.v_lim = q.v_lim; o.W_lim = q.W_lim;
  o.x_lim_f = (float)q.x_lim; o.x_lim_up = round_up_to_float(q.x_lim); o.v_lim_up = round_up_to_float(q.v_lim);
  const double lim = q.euler_lim_deg * kPi / 180.0;
  o.sin_euler_lim = sin(lim); o.tan_euler_lim = tan(lim); o.udm = (float)q.udm_fraction;
  o.reset_v = (float)(q.v_lim * 0.5); o.reset_W = (float)(q.W_lim * 0.5);
  const double rmin_mono = -ceil(q.Cx + q.CIx + q.Cv + q.Cb1 + q.CIb1 + q.CW);  // quad.py:81
  const double rmin_1 = -ceil(q.Cx + q.CIx + q.Cv + q.Cw12);                    // quad.py:85
  const double rmin_2 = -ceil(q.Cb1 + q.CW3 + q.CIb1);                          // quad.py:88
  o.rmin_mono = (float)rmin_mono; o.rmin_1 = (float)rmin_1; o.rmin_2 = (float)rmin_2;
  o.inv_x_lim = 1.0 / q.x_lim; o.inv_v_lim = 1.0 / q.v_lim; o.inv_W_lim = 1.0 / q.W_lim;
  o.inv_eIx_lim = (float)(1.0 / q.eIx_lim); o.inv_eIb1_lim = (float)(1.0 / q.eIb1_lim);
  o.inv_nrmin_mono = (float)(-1.0 / rmin_mono); o.inv_nrmin_1 = (float)(-1.0 / rmin_1); o.inv_nrmin_2 = (float)(-1.0 / rmin_2);
  const double nom[6] = {q.m_nominal, q.d_nominal, q.J1_nominal, q.J3_nominal, q.c_tf_nominal, q.c_tw_nominal};
  for (int j = 0; j < 6; ++j) { o.nom[j] = nom[j]; o.nom_f[j] = (float)nom[j]; }
  o.g = q.g; o.g_f = (float)q.g; o.min_force = q.min_force;
  const double T8 = q.eight_T > 0 ? q.eight_T : 9.0;
  o.e8_w1 = (float)(2.0 * kPi / T8); o.e8_w2 = (float)(4.0 * kPi / T8);                // :102-103
  o.e8_k = (float)(-log(q.eight_eps > 0 ? q.eight_eps : 0.01) / T8);                   // :107-108
  o.e8_A1 = (float)q.eight_A1; o.e8_A2 = (float)q.eight_A2; o.e8_wb = (float)q.eight_w_b1d; o.e8_alt = (float)q.eight_alt_d;
  o.e8_tmax = (float)(q.eight_count * T8);                                             // :436
  o.inv_w_adapt = q.w_adapt > 0 ? 1.0 / q.w_adapt : 0.0;
}

static int fill_env(Args& a, const QrEnv* e) {
  if (!e) return QR_E_NULL;
  if (e->kind < 0 || e->kind > 2 || e->layout < 0 || e->layout > 2) return QR_E_KIND;
  if (e->num_envs < 0 || (e->field_stride != 0 && (e->field_stride < e->num_envs || (e->field_stride & 3)))) return QR_E_SIZE;
  if ((e->field_stride > 0 ? e->field_stride : e->num_envs) > (int64_t)0x7fffffff / (12 * 8)) return QR_E_SIZE;  // SoA buffers < 2 GiB (32-bit buffer offsets)
  if (e->goal_mode < 0 || e->goal_mode > QR_GOAL_MODE5) return QR_E_KIND;
  if (e->goal_mode != QR_GOAL_EXTERNAL && !e->traj) return QR_E_NULL;
  if (e->goal_mode >= QR_GOAL_MODE2 && !e->goal) return QR_E_NULL;  // the stateful modes keep xd, vd, b1d, Wd there
  if (!e->pos_vel || !e->att_rate) return QR_E_NULL;
  const QrCoeffs& q = e->coeffs;
  if (!(q.m_nominal > 0 && q.d_nominal > 0 && q.J1_nominal > 0 && q.J3_nominal > 0 && q.c_tf_nominal > 0 && q.c_tw_nominal > 0 &&
        q.g > 0 && q.min_force >= 0 && q.dt > 0)) return QR_E_SIZE;  // a zero-initialised QrCoeffs: call qr_default_coeffs first
  if ((reinterpret_cast<uintptr_t>(e->pos_vel) | reinterpret_cast<uintptr_t>(e->att_rate)) & 15u) return QR_E_ALIGN;
  a.pos_vel = e->pos_vel; a.att_rate = e->att_rate; a.integ = e->integ; a.params = e->params; a.goal = e->goal;
  a.traj = e->traj; a.goal_mode = e->goal_mode;
  a.episode = e->episode; a.steps = e->steps; a.reset_count = e->reset_count;
  a.n = e->num_envs; a.ld = e->field_stride > 0 ? e->field_stride : e->num_envs;
  a.env_offset = e->env_offset; a.seed = e->seed;
  a.max_episode_steps = e->max_episode_steps; a.flags = e->flags;
  fill_coeffs(a.c, e->coeffs);
  return 0;
}

// Workgroup size: one wavefront per workgroup at every batch size.  Small batches: every SIMD
// gets a wave (N = 65 536 -> 1024 workgroups) and the LDS transposes need no cross-wave
// barrier.  Large batches: measured faster than 256-thread workgroups too (1 M envs: 38.7 vs
// 42.5 us Quad-v0, 82 vs 114 us Decoupled) — the dispatcher's ~3.6 workgroups/ns is far above
// what a bandwidth-bound launch needs, and barriers of 4-wave groups at 1-2 waves/SIMD stall.
static inline int pick_block(int64_t) { return 64; }

// The launch rule's thresholds.  The compiled-in defaults are crossovers measured on the pool's MI355X boxes (the comments at
// kHelperGrid*); boxes differ by 7-10 % in what they stream, and the wrappers' crossover moves with where the action rows come
// from, so every threshold can be overridden per process — environment variables of the same names, read once — and per env
// through QrEnv.flags (QR_FLAG_FORCE_HELPER / QR_FLAG_NO_HELPER: what QuadVecEnv(autotune=True) sets after timing both
// instantiations for ITS kind, size, box and action source).  No choice changes a result bit
// (tests/test_gpu_parity.py: test_helper_wave_launch_equals_the_plain_one, test_launch_rule_overrides_change_no_bit).
struct Tuning {
  unsigned helper_grid, helper_grid_wrap, helper_grid_rollout;
};
static unsigned env_uint(const char* name, unsigned dflt) {
  const char* v = getenv(name);
  if (!v || !*v) return dflt;
  char* end = nullptr;
  const unsigned long x = strtoul(v, &end, 10);
  return (end && *end == 0) ? (unsigned)x : dflt;
}
static const Tuning& tuning() {
  static const Tuning t = [] {
    Tuning x;
    x.helper_grid = env_uint("QR_HELPER_GRID", kHelperGrid);
    x.helper_grid_wrap = env_uint("QR_HELPER_GRID_WRAP", x.helper_grid < kHelperGridWrap ? x.helper_grid : kHelperGridWrap);
    x.helper_grid_rollout = env_uint("QR_HELPER_GRID_ROLLOUT", x.helper_grid < kHelperGridRollout ? x.helper_grid : kHelperGridRollout);
    return x;
  }();
  return t;
}

// Which instantiation a launch gets (shared by launch_kind and qr_step_kernel_info).
// (in regime for sure: done envs are re-sampled — in the launch, or, between two ONE-STEP launches, by the caller
// (QR_FLAG_CALLER_RESETS: a promise nobody can keep between the steps of a multi-step launch, which therefore ignores it))
static inline bool wants_adapt(const Args& a) {
  const bool resampled = (a.flags & QR_FLAG_AUTO_RESET) || ((a.flags & QR_FLAG_CALLER_RESETS) && a.n_steps == 1);
  return a.c.inv_w_adapt > 0 && (!resampled || a.c.inv_w_adapt * a.c.W_lim * 2.5 > 1.0);
}
static inline bool helper_choice(const Args& a, unsigned tiles, unsigned limit) {  // (the instantiation exists: rule, or the env's override for this launch family)
  const bool multi = a.n_steps > 1 || a.act_out != nullptr;
  if (a.flags & (multi ? QR_FLAG_NO_HELPER_ROLLOUT : QR_FLAG_NO_HELPER)) return false;
  if (a.flags & (multi ? QR_FLAG_FORCE_HELPER_ROLLOUT : QR_FLAG_FORCE_HELPER)) return true;
  return tiles <= limit;
}
static inline bool wants_helper(const Args& a, int kind, int layout, unsigned tiles_of_launch = 0) {  // a helper wave per tile (HELP)
  const unsigned tiles = tiles_of_launch ? tiles_of_launch : (unsigned)((a.n + 63) / 64);
  // (the multi-step instantiations hold the loop's state across steps: 181-216 VGPRs = two waves per SIMD, so a stepping
  // and a helper wave per tile are all resident only up to 1024 tiles; beyond, measured: Quad-v0 98 304 envs 3.52 against
  // 2.97 us per env-step plain, Coupled 5.06 against 3.74)
  const Tuning& tn = tuning();
  const unsigned quad_limit = a.substeps <= 1 || tn.helper_grid < kHelperGridSubsteps ? tn.helper_grid : kHelperGridSubsteps;
  // (2560 measured with one substep only.  Several substeps — since round 6 the Magnus substep — re-measured, profiles/r06/
  //  ab_magnus_helper_sweep.txt: the wrappers' helper launch is ahead up to 1664 tiles (x 2 / x 4: -6...7 %), level at 1792, behind
  //  from 1920 on (2048 tiles: +5...15 %); Quad-v0 keeps kHelperGridSubsteps = 2560.)
  const unsigned wrap_limit = a.substeps <= 1 || tn.helper_grid_wrap < kHelperGridWrapSubsteps ? tn.helper_grid_wrap : kHelperGridWrapSubsteps;
  const unsigned limit = a.n_steps > 1 ? tn.helper_grid_rollout : (kind == QR_KIND_QUAD ? quad_limit : wrap_limit);
  return layout == QR_LAYOUT_MIXED && a.act_out == nullptr && a.goal_mode == QR_GOAL_EXTERNAL && !wants_adapt(a) &&
         (a.flags & QR_FLAG_AUTO_RESET) && helper_choice(a, tiles, limit);
}

static inline bool wants_helper_traj(const Args& a, int kind) {  // the same with the fused goal generator (one-step launches)
  const unsigned tiles = (unsigned)((a.n + 63) / 64);
  const Tuning& tn = tuning();
  const unsigned wrap_traj = a.substeps <= 1 ? 2048u : kHelperGridWrapSubsteps;
  return a.act_out == nullptr && a.goal_mode != QR_GOAL_EXTERNAL && a.goal_mode < QR_GOAL_MODE2 && !wants_adapt(a) && (a.flags & QR_FLAG_AUTO_RESET) &&
         helper_choice(a, tiles, kind == QR_KIND_QUAD ? (tn.helper_grid < kHelperGridSubsteps ? tn.helper_grid : kHelperGridSubsteps)
                                                      : (tn.helper_grid_wrap < wrap_traj ? tn.helper_grid_wrap : wrap_traj));
}

// qr_rollout_actor beyond the grid on which a stepping AND a helper wave per tile are all resident: instead of the plain
// instantiation over the whole grid, the helper-wave instantiation over chunks of that many tiles, one launch after the other (each
// runs all n_steps of its envs; results do not depend on the split).  Measured, profiles/r05/ab_chunked_rollouts.txt: Coupled PPO
// collection 98 304 / 131 072 / 262 144 envs 8.00 / 8.13 / 16.3 -> 6.28 / 6.40 / 13.3 us per env-step, Decoupled 262 144 18.1 -> 14.1.
// Not for the plain rollouts, whose two stepping waves per SIMD use the vector unit better than chunks do (Coupled 262 144: 6.77
// against 7.60 us chunked).
static inline unsigned rollout_chunk(const Args& a, int kind, int layout) {
  const unsigned tiles = (unsigned)((a.n + 63) / 64), limit = tuning().helper_grid_rollout;
  if (a.act_out == nullptr || kind == QR_KIND_QUAD || layout != QR_LAYOUT_MIXED || tiles <= limit || limit == 0) return 0;
  if ((a.flags & QR_FLAG_NO_HELPER_ROLLOUT) || !(a.flags & QR_FLAG_AUTO_RESET) || a.goal_mode != QR_GOAL_EXTERNAL) return 0;
  return limit;
}

// ------------------------------------------------------------------------------------
// Which instantiation of step_kernel a launch gets: ONE function decides (launch_kind dispatches on its result, qr_launch_plan
// reports it), and ONE table (QR_INSTANCES) lists every instantiation that exists.
// ------------------------------------------------------------------------------------
struct Pick {
  int traj; bool adapt; int policy; bool single, help, hrew, mag = false;
  // the bits qr_launch_stats counts under (with layout << 16 | kind << 8; MAG is bit 12, above the kind's two bits)
  unsigned bits() const {
    return (unsigned)traj | (adapt ? 4u : 0u) | ((unsigned)policy << 3) | (single ? 32u : 0u) | (help ? 64u : 0u) | (hrew ? 128u : 0u) | (mag ? 0x1000u : 0u);
  }
  unsigned slot() const { return (bits() & 0xFFu) | (mag ? 0x100u : 0u); }   // index into the counters
};

// `tiles_of_launch` != 0: one chunk of a chunked qr_rollout_actor (rollout_chunk).
static inline Pick pick_shape(const Args& a, int kind, int layout, unsigned tiles_of_launch) {
  const bool mixed = layout == QR_LAYOUT_MIXED;  // the only layout with one-step (SINGLE) and helper-wave (HELP) instantiations
  const unsigned tiles = tiles_of_launch ? tiles_of_launch : (unsigned)((a.n + 63) / 64);
  // Rate adaptivity can only trigger when an env starts a step with max|W_i| > w_adapt.  With
  // AUTO_RESET every env whose rate error left its bound was re-sampled at the end of the step
  // that took it there (done): Quad-v0 |W_i| < W_lim, Coupled |W_i - Wd_i| < W_lim, Decoupled
  // |W - Wd| < 2 W_lim (|ew12_i| < W_lim and |eW3| < W_lim).  For goal rates |Wd| <= W_lim / 2
  // and w_adapt >= 2.5 W_lim (the default 16 rad/s is) the plain kernel computes the same bits.
  const bool adapt = wants_adapt(a);
  const bool traj = a.goal_mode != QR_GOAL_EXTERNAL, stateful = a.goal_mode >= QR_GOAL_MODE2;
  if (kind != QR_KIND_QUAD && a.act_out != nullptr) {  // ---- qr_rollout_actor ----
    const bool general = a.actor[0].ls_w || a.actor[0].squash != QR_ACTOR_TANH_MEAN ||
                         (kind == QR_KIND_DECOUPLED && (a.actor[1].ls_w || a.actor[1].squash != QR_ACTOR_TANH_MEAN));
    if (mixed) {
      // Actors with in-launch resets and external goals, on grids where every wave is resident: a helper wave
      // per tile (noise, reset pool, observation rows).  Measured, Coupled 65 536 envs, T = 32: 5.37 -> 4.51 us per step;
      // with the fused goal generator the same split measured SLOWER (5.65 -> 6.25 us per step, tools/ppo_rollout_bench.py;
      // both waves of a tile must be resident, which caps the kernel at 256 registers) and is not instantiated.
      // Stage arithmetic: like every other launch, the plain (non-adaptive) instantiation whenever adaptivity provably cannot
      // trigger (in-launch resets, w_adapt >= 2.5 W_lim) — the actor rollout then computes the same bits as qr_step on the
      // actions it sampled, and the delta-form stages are off its path (65 536 envs: 3.70 -> 3.56 us per env-step,
      // profiles/r05/ab_actor_plain.txt).  External goals only: with the fused generator the actor launches stay rate-adaptive.
      // (the general form — SAC's log_std head and rule — with the same split; measured, profiles/r05/ab_sac_helper.txt,
      //  65 536 envs, T = 32: Coupled 4.95 -> 4.38 us per env-step, Decoupled 5.54 -> 4.87, bit-identical)
      if (!traj && (a.flags & QR_FLAG_AUTO_RESET) && helper_choice(a, tiles, tuning().helper_grid_rollout))
        return {0, adapt, general ? 2 : 1, false, true, true};
      if (!traj && !adapt) return {0, false, general ? 2 : 1, false, false, true};
    }
    if (stateful) return {2, true, 2, false, false, true};  // stateful goal modes: the general actor form
    return {traj ? 1 : 0, true, general ? 2 : 1, false, false, true};
  }
  const bool help = mixed && wants_helper(a, kind, QR_LAYOUT_MIXED, tiles_of_launch);
  if (mixed && a.n_steps == 1) {  // ---- qr_step in the default layout: the instantiations without the loop over env-steps ----
    if (stateful) return {2, adapt, 0, true, false, true};  // take-off, landing, stay, circle: their own instantiations
    if (traj) {
      if (adapt) return {1, true, 0, true, false, true};
      return {1, false, 0, true, wants_helper_traj(a, kind), true};  // (fused goal generator + helper wave: one-step launches only)
    }
    if (adapt) return {0, true, 0, true, false, true};
    if (help) {
      // (Quad-v0, one substep, more than kHelpRewardTiles tiles: the reward stays on the stepping wave — measured with the
      //  product's other choices in place, profiles/r05/ab_step_prio.txt: 98 304 envs 5.12 -> 4.92 us, 163 840 envs 7.31 -> 6.57;
      //  identical bits.  The wrappers, one substep, more than kHelpRowsTiles tiles: the helper only samples the pool, the
      //  rows go out with the stepping wave — 114 688 envs Coupled 8.14 -> 6.98 us, Decoupled 8.21 -> 6.97; 131 072: 9.07 -> 8.61 /
      //  9.11 -> 8.69; 98 304 envs and below are better with the helper's rows; profiles/r05/ab_step_prio.txt)
      const unsigned lim = kind == QR_KIND_QUAD ? kHelpRewardTiles : kHelpRowsTiles;
      return {0, false, 0, true, true, !(a.substeps == 1 && tiles > lim)};
    }
    return {0, false, 0, true, false, true};
  }
  // ---- qr_rollout (any layout) and qr_step of the uniform layouts ----
  if (stateful) return {2, adapt, 0, false, false, true};
  if (traj) return {1, adapt, 0, false, false, true};
  if (adapt) return {0, true, 0, false, false, true};
  return {0, false, 0, false, help, true};  // (rollouts in the default layout: a helper wave per tile for grids it pays on)
}

// The integrator rides on the env's `substeps` alone — never on the grid, so that a shard computes the bits of the global batch:
// two or more substeps in the default layout take the Magnus substep (MAG; qr_dynamics.h: 74 instead of 149 instructions per
// substep), one substep keeps RK4 in kernels that hold nothing else (byte-identical to the build without MAG).  The rate-adaptive
// delta-form instantiations (ADAPT without an actor: the launches whose envs may leave the regime) have their own arithmetic.
static constexpr bool uses_plain_integrate(int adapt, int policy) { return !adapt || policy; }
static inline Pick pick_instance(const Args& a, int kind, int layout, unsigned tiles_of_launch = 0) {
  Pick p = pick_shape(a, kind, layout, tiles_of_launch);
  p.mag = layout == QR_LAYOUT_MIXED && a.substeps >= 2 && uses_plain_integrate(p.adapt, p.policy);
  return p;
}

// Every instantiation: (TRAJ, ADAPT, POLICY, SINGLE, HELP, HREW) x MAG.  POLICY != 0 exists for the wrappers only; SINGLE, HELP and the
// non-adaptive actor rollouts for the default layout only (inst_exists) — 16 Quad-v0 + 2 x 27 wrapper kernels in the default
// layout, 6 + 2 x 11 in each uniform one; MAG = 1 twins of the default layout's rows that call `integrate` (all but the delta-form
// ones and the one-substep-only HREW = 0 rows): 9 Quad-v0 + 2 x 20.  175 in all.  tests/test_gpu_instances.py walks this table and checks that the suite launches all of it.
#define QR_INSTANCES(X)                                                                                                  \
  X(0, 0, 0, 0, 0, 1) X(0, 1, 0, 0, 0, 1) X(1, 0, 0, 0, 0, 1) X(1, 1, 0, 0, 0, 1) X(2, 0, 0, 0, 0, 1) X(2, 1, 0, 0, 0, 1) \
  X(0, 1, 1, 0, 0, 1) X(0, 1, 2, 0, 0, 1) X(1, 1, 1, 0, 0, 1) X(1, 1, 2, 0, 0, 1) X(2, 1, 2, 0, 0, 1)                     \
  X(0, 0, 1, 0, 0, 1) X(0, 0, 2, 0, 0, 1) X(0, 0, 1, 0, 1, 1) X(0, 1, 1, 0, 1, 1) X(0, 0, 2, 0, 1, 1) X(0, 1, 2, 0, 1, 1) \
  X(0, 0, 0, 0, 1, 1)                                                                                                    \
  X(0, 0, 0, 1, 0, 1) X(0, 1, 0, 1, 0, 1) X(1, 0, 0, 1, 0, 1) X(1, 1, 0, 1, 0, 1) X(2, 0, 0, 1, 0, 1) X(2, 1, 0, 1, 0, 1) \
  X(1, 0, 0, 1, 1, 1) X(0, 0, 0, 1, 1, 1) X(0, 0, 0, 1, 1, 0)
static constexpr bool inst_exists(int kind, bool mixed, int tr, int ad, int po, int si, int he, int hr, int mg = 0) {
  (void)tr;
  // (MAG: the default layout's rows that call `integrate`; HREW = 0 is a one-substep choice, pick_shape)
  return !(po != 0 && kind == QR_KIND_QUAD) && (mixed || !(si || he || (po != 0 && !ad))) && (!mg || (mixed && uses_plain_integrate(ad, po) && hr));
}
// (a consumer of the table defines QR_X1 with the seventh column, MAG)
#define QR_X(TR, AD, PO, SI, HE, HR) QR_X1(TR, AD, PO, SI, HE, HR, 0) QR_X1(TR, AD, PO, SI, HE, HR, 1)

// Host-side launch counters, one per (layout, kind, instantiation): which kernels a process really ran (qr_launch_stats).
static std::atomic<uint32_t> g_launches[3][3][512];

template <int KIND, typename XV, typename QW>
static int launch_kind(const Args& a, hipStream_t s, unsigned tiles_of_launch = 0) {
  constexpr bool kMixed = std::is_same<XV, float>::value && std::is_same<QW, double>::value;
  constexpr int kLayout = kMixed ? QR_LAYOUT_MIXED : (std::is_same<XV, double>::value ? QR_LAYOUT_F64 : QR_LAYOUT_F32);
  if constexpr (kMixed) {
    if (tiles_of_launch == 0) {
      if (const unsigned chunk = rollout_chunk(a, KIND, QR_LAYOUT_MIXED)) {
        const unsigned tiles = (unsigned)((a.n + 63) / 64);
        for (unsigned base = 0; base < tiles; base += chunk) {
          Args b = a;
          b.tile_base = (int32_t)base;
          if (int rc = launch_kind<KIND, XV, QW>(b, s, tiles - base < chunk ? tiles - base : chunk)) return rc;
        }
        return 0;
      }
    }
  }
  const dim3 grid(tiles_of_launch ? tiles_of_launch : (unsigned)((a.n + 63) / 64));
  const Pick p = pick_instance(a, KIND, kLayout, tiles_of_launch);
#define QR_STEP_ARGS a.pos_vel, a.att_rate, a.action, a.params, a.integ, ((a.flags & QR_FLAG_AUTO_RESET) ? a.reset_count : nullptr), (int32_t)a.n, (int32_t)a.ld, a
#define QR_X1(TR, AD, PO, SI, HE, HR, MG)                                                                                         \
  if constexpr (inst_exists(KIND, kMixed, TR, AD, PO, SI, HE, HR, MG)) {                                                          \
    if (p.traj == TR && p.adapt == (bool)AD && p.policy == PO && p.single == (bool)SI && p.help == (bool)HE && p.hrew == (bool)HR && \
        p.mag == (bool)MG) {                                                                                                      \
      g_launches[kLayout][KIND][p.slot()].fetch_add(1u, std::memory_order_relaxed);                                              \
      hipLaunchKernelGGL((step_kernel<KIND, XV, QW, 64, TR, (bool)AD, PO, (bool)SI, (bool)HE, (bool)HR, (bool)MG>), grid, dim3(HE ? 128 : 64), 0, s, QR_STEP_ARGS); \
      return 0;                                                                                                                   \
    }                                                                                                                             \
  }
  QR_INSTANCES(QR_X)
#undef QR_X1
#undef QR_STEP_ARGS
  return QR_E_KIND;  // (unreachable: pick_instance only returns rows of the table)
}

// QR_ONLY_KIND / QR_ONLY_LAYOUT: experiment builds that instantiate one env kind / one layout only
// (seconds instead of a minute to compile; tools/ab_libs.py); the product build has neither.
template <typename XV, typename QW>
static int launch_step(const Args& a, int kind, hipStream_t s) {
  if (a.n == 0) return 0;
#ifdef QR_ONLY_KIND
  if (kind != QR_ONLY_KIND) return QR_E_KIND;
  int rc = launch_kind<QR_ONLY_KIND, XV, QW>(a, s);
#else
  int rc = 0;
  switch (kind) {
    case QR_KIND_QUAD: rc = launch_kind<QR_KIND_QUAD, XV, QW>(a, s); break;
    case QR_KIND_COUPLED: rc = launch_kind<QR_KIND_COUPLED, XV, QW>(a, s); break;
    default: rc = launch_kind<QR_KIND_DECOUPLED, XV, QW>(a, s); break;
  }
#endif
  return rc ? rc : (int)hipGetLastError();
}

#ifdef QR_ONLY_LAYOUT
#define QR_DISPATCH_LAYOUT(layout, CALL) { using XV = float; using QW = double; CALL; }
#else
#define QR_DISPATCH_LAYOUT(layout, CALL)                                        \
  switch (layout) {                                                             \
    case QR_LAYOUT_MIXED: { using XV = float; using QW = double; CALL; } break; \
    case QR_LAYOUT_F64:   { using XV = double; using QW = double; CALL; } break; \
    default:              { using XV = float; using QW = float; CALL; } break;  \
  }
#endif

// The tail of the C-ABI's one-kernel entry points: one 64-lane workgroup per 64-env tile on the caller's stream.
// launch(XV(), QW(), grid, stream) starts the kernel for the env's layout (its first two arguments carry the types).
template <typename F>
static int launch_tiles(const Args& a, int layout, void* stream, F launch) {
  const unsigned grid = (unsigned)((a.n + 63) / 64);
  if (grid == 0) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  (void)layout;
  QR_DISPATCH_LAYOUT(layout, (launch(XV(), QW(), dim3(grid), s)));
  return (int)hipGetLastError();
}

static int fill_actor(ActorW& w, const QrActor& q, int obs_dim, int hidden, int action_dim) {
  if (q.obs_dim != obs_dim || q.hidden_dim != hidden || q.action_dim != action_dim) return QR_E_SIZE;
  if (!q.fc1_w || !q.fc1_b || !q.fc2_w || !q.fc2_b || !q.mean_w || !q.mean_b) return QR_E_NULL;
  if (!q.log_std && !(q.log_std_w && q.log_std_b)) return QR_E_NULL;  // one of the two log_std sources
  if ((q.log_std_w == nullptr) != (q.log_std_b == nullptr)) return QR_E_NULL;
  if (q.squash != QR_ACTOR_TANH_MEAN && q.squash != QR_ACTOR_TANH_SAMPLE) return QR_E_KIND;
  w.fc1_w = q.fc1_w; w.fc1_b = q.fc1_b; w.fc2_w = q.fc2_w; w.fc2_b = q.fc2_b;
  w.mean_w = q.mean_w; w.mean_b = q.mean_b; w.log_std = q.log_std;
  w.ls_w = q.log_std_w; w.ls_b = q.log_std_b; w.squash = q.squash;
  return 0;
}

static int do_rollout(const QrEnv* env, const float* action, const QrPolicyRollout* pol, int32_t n_steps, int32_t substeps,
                      const QrStepOut* out, void* stream) {
  Args a{};
  if (int rc = fill_env(a, env)) return rc;
  if ((!action && !pol) || !out || !out->reward || !out->done) return QR_E_NULL;
  if (substeps < 1 || n_steps < 1) return QR_E_SIZE;
  if (env->kind != QR_KIND_QUAD && (!env->integ || !out->obs0)) return QR_E_NULL;
  if (env->kind == QR_KIND_DECOUPLED && !out->obs1) return QR_E_NULL;
  if ((env->flags & QR_FLAG_AUTO_RESET) && (!env->episode || !env->reset_count)) return QR_E_NULL;
  if (env->kind == QR_KIND_DECOUPLED && out->final_obs0 && !out->final_obs1) return QR_E_NULL;
  if (pol) {
    if (env->kind == QR_KIND_QUAD) return QR_E_KIND;
    if (!pol->actors || !pol->obs0_in || !pol->action_out) return QR_E_NULL;
    if (env->kind == QR_KIND_COUPLED) {
      if (int rc = fill_actor(a.actor[0], pol->actors[0], 23, 16, 4)) return rc;
    } else {
      if (!pol->obs1_in) return QR_E_NULL;
      if (int rc = fill_actor(a.actor[0], pol->actors[0], 15, 16, 4)) return rc;
      if (int rc = fill_actor(a.actor[1], pol->actors[1], 3, 4, 1)) return rc;
    }
    const uintptr_t amask = env->kind == QR_KIND_DECOUPLED ? 3u : 15u;  // A = 4: one 16-byte store per lane
    if ((reinterpret_cast<uintptr_t>(pol->action_out) | reinterpret_cast<uintptr_t>(pol->logprob_out)) & amask) return QR_E_ALIGN;
    if (!(pol->max_action > 0.0f)) return QR_E_SIZE;
    a.obs0_in = pol->obs0_in; a.obs1_in = pol->obs1_in; a.noise = pol->noise;
    a.act_out = pol->action_out; a.logp_out = pol->logprob_out;
    a.noise_seed = pol->noise_seed; a.step_base = pol->step_base;
    a.max_action = pol->max_action; a.deterministic = pol->deterministic;
  } else {
    // action rows: A = 4 is read with one 16-byte load per lane; A = 5 (DECOUPLED) with dword loads
    if (reinterpret_cast<uintptr_t>(action) & (env->kind == QR_KIND_DECOUPLED ? 3u : 15u)) return QR_E_ALIGN;
  }
  a.action = action; a.obs0 = out->obs0; a.obs1 = out->obs1; a.final_obs0 = out->final_obs0; a.final_obs1 = out->final_obs1;
  a.reward = out->reward; a.reward_raw = out->reward_raw; a.done = out->done; a.truncated = out->truncated;
  a.n_steps = n_steps; a.substeps = substeps;
#ifdef QR_SPAN
  a.span_slot = g_span_slot; a.span_buf = g_span_buf;
#endif
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  int rc = 0;
  QR_DISPATCH_LAYOUT(env->layout, (rc = launch_step<XV, QW>(a, env->kind, s)));
  return rc;
}

// qr_evaluate_actor: eval_kernel over the whole grid, one 64-env tile per workgroup.  Instantiations: both wrappers x TRAJ 0 / 1 / 2 x
// (default layout: RK4 and Magnus; uniform layouts: RK4) = 24, none of them a step_kernel (not in QR_INSTANCES, not counted by
// qr_launch_stats).  The integrator follows pick_instance's rule for a plain actor rollout: Magnus for two or more substeps in the
// default layout.  qr_evaluate_population launches the same kernels: which policy a tile flies is data (EvalArgs), not an instantiation.
template <int KIND, typename XV, typename QW>
static void launch_eval_kind(const EvalLaunch& k, hipStream_t s) {
  constexpr bool kMixed = std::is_same<XV, float>::value && std::is_same<QW, double>::value;
  const dim3 grid((unsigned)((k.a.n + 63) / 64));
  const int traj = k.a.goal_mode == QR_GOAL_EXTERNAL ? 0 : (k.a.goal_mode >= QR_GOAL_MODE2 ? 2 : 1);
  const bool mag = kMixed && k.a.substeps >= 2 && uses_plain_integrate(0, 1);
#define QR_EVAL(TR, MG) hipLaunchKernelGGL((eval_kernel<KIND, XV, QW, TR, MG>), grid, dim3(64), 0, s, k)
  if constexpr (kMixed) {
    if (mag) {
      if (traj == 0) QR_EVAL(0, true); else if (traj == 1) QR_EVAL(1, true); else QR_EVAL(2, true);
      return;
    }
  }
  if (traj == 0) QR_EVAL(0, false); else if (traj == 1) QR_EVAL(1, false); else QR_EVAL(2, false);
#undef QR_EVAL
}

template <typename XV, typename QW>
static int launch_eval(const EvalLaunch& k, int kind, hipStream_t s) {
  if (k.a.n == 0) return 0;
#ifdef QR_ONLY_KIND
  if constexpr (QR_ONLY_KIND == QR_KIND_QUAD) {
    return QR_E_KIND;
  } else {
    if (kind != QR_ONLY_KIND) return QR_E_KIND;
    launch_eval_kind<QR_ONLY_KIND, XV, QW>(k, s);
  }
#else
  if (kind == QR_KIND_COUPLED) launch_eval_kind<QR_KIND_COUPLED, XV, QW>(k, s);
  else launch_eval_kind<QR_KIND_DECOUPLED, XV, QW>(k, s);
#endif
  return (int)hipGetLastError();
}

// `pop` == NULL: qr_evaluate_actor, one policy over all N envs.  Otherwise qr_evaluate_population's block layout (quadrotor_hip.h).
static int do_evaluate(const QrEnv* env, const QrPolicyRollout* pol, const QrPopulation* pop, int32_t max_steps, int32_t substeps,
                       const QrEvalOut* out, void* stream) {
  EvalLaunch k{};
  Args& a = k.a;
  if (int rc = fill_env(a, env)) return rc;
  if (!pol || !out) return QR_E_NULL;
  const int64_t tiles = (a.n + 63) / 64;
  k.e.envs_per_policy = (int32_t)a.n; k.e.tiles_per_policy = (int32_t)(tiles > 0 ? tiles : 1);
  if (pop) {
    if (pop->n_policies < 1 || pop->envs_per_policy < 1) return QR_E_SIZE;
    const int64_t tpp = ((int64_t)pop->envs_per_policy + 63) / 64;
    if (a.n != (int64_t)pop->n_policies * tpp * 64) return QR_E_SIZE;
    k.e.envs_per_policy = pop->envs_per_policy; k.e.tiles_per_policy = (int32_t)tpp;
  }
  if (env->kind == QR_KIND_QUAD) return QR_E_KIND;
  if (substeps < 1 || max_steps < 1) return QR_E_SIZE;
  if (!env->integ || !pol->actors || !pol->obs0_in || !out->obs0 || !out->episode_return || !out->benchmark || !out->length ||
      !out->terminated || !out->success) return QR_E_NULL;
  if (env->kind == QR_KIND_COUPLED) {
    if (int rc = fill_actor(a.actor[0], pol->actors[0], 23, 16, 4)) return rc;
  } else {
    if (!pol->obs1_in || !out->obs1) return QR_E_NULL;
    if (int rc = fill_actor(a.actor[0], pol->actors[0], 15, 16, 4)) return rc;
    if (int rc = fill_actor(a.actor[1], pol->actors[1], 3, 4, 1)) return rc;
  }
  if (!(pol->max_action > 0.0f)) return QR_E_SIZE;
  for (ActorW& w : a.actor) w.log_std = w.ls_w = w.ls_b = nullptr;  // the deterministic rule reads no log_std
  a.obs0_in = pol->obs0_in; a.obs1_in = pol->obs1_in; a.act_out = pol->action_out; a.max_action = pol->max_action;
  a.obs0 = out->obs0; a.obs1 = out->obs1;
  a.n_steps = max_steps; a.substeps = substeps;
  EvalArgs& e = k.e;
  e.ret = out->episode_return; e.bench = out->benchmark; e.length = out->length; e.terminated = out->terminated;
  e.success = out->success; e.final_error = out->final_error; e.max_steps = max_steps;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  int rc = 0;
  QR_DISPATCH_LAYOUT(env->layout, (rc = launch_eval<XV, QW>(k, env->kind, s)));
  return rc;
}

// qr_adamw_step: every argument check, then ONE launch of n_groups workgroups.  Nothing is launched on an error.
static int do_adamw(const QrAdamWGroup* groups, int32_t n_groups, void* stream) {
  if (!groups) return QR_E_NULL;
  if (n_groups < 1 || n_groups > kAdamWGroups) return QR_E_SIZE;
  AdamWArgs a{};
  for (int i = 0; i < n_groups; ++i) {
    const QrAdamWGroup& g = groups[i];
    AdamWGroupArgs& d = a.g[i];
    if (g.n_tensors < 1 || g.n_tensors > kAdamWTensors) return QR_E_SIZE;
    int64_t total = 0;
    for (int k = 0; k < g.n_tensors; ++k) {
      if (g.count[k] < 1) return QR_E_SIZE;
      total += g.count[k];
    }
    if (total > kAdamWMaxEntries) return QR_E_SIZE;
    const double nonneg[] = {g.lr, g.eta_min, (double)g.eps, (double)g.weight_decay};
    for (double v : nonneg)
      if (!(v >= 0.0) || !(v <= 1.79769313486231570e308)) return QR_E_SIZE;
    if (!(g.beta1 >= 0.0f && g.beta1 < 1.0f) || !(g.beta2 >= 0.0f && g.beta2 < 1.0f) || g.t0 < 0 || g.max_norm != g.max_norm) return QR_E_SIZE;
    if (!g.exp_avg || !g.exp_avg_sq || !g.step) return QR_E_NULL;
    for (int k = 0; k < g.n_tensors; ++k)
      if (!g.param[k] || !g.grad[k]) return QR_E_NULL;
    uintptr_t bits = reinterpret_cast<uintptr_t>(g.exp_avg) | reinterpret_cast<uintptr_t>(g.exp_avg_sq) | reinterpret_cast<uintptr_t>(g.stats);
    for (int k = 0; k < g.n_tensors; ++k) bits |= reinterpret_cast<uintptr_t>(g.param[k]) | reinterpret_cast<uintptr_t>(g.grad[k]);
    if ((bits & 3u) || (reinterpret_cast<uintptr_t>(g.step) & 7u)) return QR_E_ALIGN;
    for (int k = 0; k < kAdamWTensors; ++k) {
      const bool used = k < g.n_tensors;
      d.param[k] = used ? g.param[k] : nullptr;
      d.grad[k] = used ? g.grad[k] : nullptr;
      d.off[k + 1] = d.off[k] + (used ? g.count[k] : 0);
    }
    d.exp_avg = g.exp_avg; d.exp_avg_sq = g.exp_avg_sq; d.step = g.step; d.stats = g.stats;
    d.lr = g.lr; d.eta_min = g.eta_min; d.t0 = g.t0;
    d.beta1 = g.beta1; d.beta2 = g.beta2; d.eps = g.eps; d.weight_decay = g.weight_decay; d.max_norm = g.max_norm;
  }
  hipLaunchKernelGGL(adamw_step_kernel, dim3((unsigned)n_groups), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  return (int)hipGetLastError();
}

// qr_adamw_polyak_step: do_adamw's checks in its order, with do_soft_update's for the targets, then ONE launch of n_groups workgroups.
// Nothing is launched on an error.
static int do_adamw_polyak(const QrAdamWPolyakGroup* groups, int32_t n_groups, void* stream) {
  if (!groups) return QR_E_NULL;
  if (n_groups < 1 || n_groups > kPolyakGroups) return QR_E_SIZE;
  AdamWPolyakArgs a{};
  for (int i = 0; i < n_groups; ++i) {
    const QrAdamWPolyakGroup& g = groups[i];
    AdamWPolyakGroupArgs& d = a.g[i];
    if (g.n_tensors < 1 || g.n_tensors > kPolyakTensors || g.reserved0 != 0) return QR_E_SIZE;
    int64_t total = 0;
    for (int k = 0; k < g.n_tensors; ++k) {
      if (g.count[k] < 1) return QR_E_SIZE;
      total += g.count[k];
    }
    if (total > kAdamWMaxEntries) return QR_E_SIZE;
    const double nonneg[] = {g.lr, g.eta_min, (double)g.eps, (double)g.weight_decay};
    for (double v : nonneg)
      if (!(v >= 0.0) || !(v <= 1.79769313486231570e308)) return QR_E_SIZE;
    if (!(g.beta1 >= 0.0f && g.beta1 < 1.0f) || !(g.beta2 >= 0.0f && g.beta2 < 1.0f) || g.t0 < 0 || g.max_norm != g.max_norm) return QR_E_SIZE;
    if (!(g.tau >= 0.0 && g.tau <= 1.0) || (g.exp_out && total != 1)) return QR_E_SIZE;
    if (!g.exp_avg || !g.exp_avg_sq || !g.step) return QR_E_NULL;
    for (int k = 0; k < g.n_tensors; ++k)
      if (!g.param[k] || !g.grad[k]) return QR_E_NULL;
    for (int k = 0; k < g.n_tensors; ++k)
      if (g.target[k] == g.param[k]) return QR_E_SIZE;
    uintptr_t bits = reinterpret_cast<uintptr_t>(g.exp_avg) | reinterpret_cast<uintptr_t>(g.exp_avg_sq) | reinterpret_cast<uintptr_t>(g.stats) |
                     reinterpret_cast<uintptr_t>(g.exp_out);
    for (int k = 0; k < g.n_tensors; ++k)
      bits |= reinterpret_cast<uintptr_t>(g.param[k]) | reinterpret_cast<uintptr_t>(g.grad[k]) | reinterpret_cast<uintptr_t>(g.target[k]);
    if ((bits & 3u) || (reinterpret_cast<uintptr_t>(g.step) & 7u)) return QR_E_ALIGN;
    for (int k = 0; k < kPolyakTensors; ++k) {
      const bool used = k < g.n_tensors;
      d.param[k] = used ? g.param[k] : nullptr;
      d.grad[k] = used ? g.grad[k] : nullptr;
      d.target[k] = used ? g.target[k] : nullptr;
      d.off[k + 1] = d.off[k] + (used ? g.count[k] : 0);
    }
    d.exp_avg = g.exp_avg; d.exp_avg_sq = g.exp_avg_sq; d.step = g.step; d.stats = g.stats; d.exp_out = g.exp_out;
    d.lr = g.lr; d.eta_min = g.eta_min; d.t0 = g.t0;
    d.beta1 = g.beta1; d.beta2 = g.beta2; d.eps = g.eps; d.weight_decay = g.weight_decay; d.max_norm = g.max_norm;
    d.tau = (float)g.tau; d.omt = (float)(1.0 - g.tau);
  }
  hipLaunchKernelGGL(adamw_polyak_kernel, dim3((unsigned)n_groups), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  return (int)hipGetLastError();
}

}  // namespace qr
