// qr_step.h — part of the gfx950 quadrotor step library (included by quadrotor_kernels.hip, in this order).
// The fused step / rollout kernel: span macros, launch thresholds, Quad-v0 reward and termination, step_kernel.
#pragma once
#include "qr_actor.h"

namespace qr {

// byte offset of the Args block in the step kernel's kernarg segment: 6 pointers + 2 x int32 precede it
[[maybe_unused]] constexpr int kArgsOffset = 6 * 8 + 2 * 4;
static_assert(alignof(Args) == 8, "Args follows the leading scalar arguments without padding");
#ifndef QR_SPAN
static_assert(sizeof(Coeffs) <= 5 * 64 && offsetof(Args, c) + sizeof(Coeffs) == sizeof(Args), "the step kernel touches the five kernarg lines of the coefficient block (the last field of Args)");
#endif

// QR_SPAN: the light diagnostic build (tools/span_timeline.py).  Every wave records the 100 MHz real-time clock twice — with its first
// instruction and behind its last — into row `span_slot` of a buffer of its own; a chain of launches with slots 0, 1, 2, ... then
// shows, on the device's own clock, each launch's SPAN (first wave in to last wave out) and the GAP to the next launch.  Two scalar
// memory-time reads per wave and one 16-byte store at the very end: the build runs within a few per cent of the product's period
// (the retired seven-stamp build: +50 %), which is what makes span + gap a usable clock for kernels rocprofv3 inflates.
#ifdef QR_SPAN
static unsigned long long* g_span_buf = nullptr;  // (host) the stamp buffer and the row the next launches write: qr_debug_set_span[_slot]
static int g_span_slot = -1;
// Buffer pointer and row come with the launch's own kernarg.  A clock read is a scalar
// memory operation whose result lands asynchronously: it is WAITED FOR on the spot (the compiler knows nothing of the pending
// write and would otherwise reuse the register pair), which costs its wave ~0.3 us.  So only a sample of the waves pays:
//   ENTRY stamps: the first eight workgroups (one per XCD; the dispatcher starts with them) — a launch's "first wave in";
//   EXIT stamps: the workgroups of every fourth tile, spread over the XCDs — a launch's "last wave out" is then a stamped one in
//   a quarter of the launches, and the chain's MEDIAN period stays within ~1 % of the product's.
// (buffer pointer and row are read from the kernarg segment by the stamped waves only, at their end and BEHIND the clock read: one more
// kernarg line requested at the kernel's start would sit in every wave's first scalar wait — 0.3 us per launch)
#define QR_SPAN_BEGIN()                                                  \
  unsigned long long span_t0_ = 0;                                       \
  if (blockIdx.x < 8u) asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(span_t0_) : : "memory")
#define QR_SPAN_END()                                                                                          \
  do {                                                                                                         \
    const bool exit_ = (((blockIdx.x >> 3) + blockIdx.x) & 3u) == 0u;                                          \
    if (exit_ || blockIdx.x < 8u) {                                                                            \
      unsigned long long t1_ = 0;                                                                              \
      if (exit_) asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t1_) : : "memory");            \
      unsigned long long* const span_buf_ = ka.span_buf;                                                       \
      const int span_slot_ = ka.span_slot;                                                                     \
      if (span_buf_ != nullptr && span_slot_ >= 0 && (threadIdx.x & 63u) == 0) {                               \
        const size_t w_ = ((size_t)span_slot_ * (((unsigned)n_envs + 63u) >> 6) + blockIdx.x) * 2 + (threadIdx.x >> 6); \
        span_buf_[2 * w_] = span_t0_; span_buf_[2 * w_ + 1] = t1_;                                             \
      }                                                                                                        \
    }                                                                                                          \
  } while (0)
#else
#define QR_SPAN_BEGIN() do { } while (0)
#define QR_SPAN_END() do { } while (0)
#endif

constexpr int kStepPrio = 3;                  // s_setprio of the stepping wave in the helper-wave launches
constexpr unsigned kHelpRewardTiles = 1408;   // one-step Quad-v0 helper launches beyond this many tiles form the reward on the stepping wave
constexpr unsigned kHelpRowsTiles = 1600;     // one-step wrapper helper launches beyond this many tiles store their rows from the stepping wave
constexpr int kPrioSubsteps = 2;
constexpr unsigned kHelperGridWrapSubsteps = 1664;  // the wrappers' one-step helper-wave launches with two or more substeps: up to this many tiles (wants_helper)
constexpr unsigned kPrioSingleTiles = 768;
constexpr int kEarlyStoreGrid = 4096;  // grids up to this many waves store a resetting wave's settled lanes before it samples (65 536 envs 5.43 / 5.49 us, 1 M 39.4 / 37.4)
// (Settled A/Bs whose losing arms are gone from the tree — the winning arm is the code, the measurement is cited where it applies:
//  kernarg lines requested with the wave's first instructions (Decoupled 5.16 -> 5.02 us), output pointers read with the first scalar
//  batch in the plain launches (1 M envs 34.7 -> 33.9 us), rows to the LDS tile before the reset block + late goal / integrator loads
//  in the plain wrapper launches (262 144 envs 19.1 -> 16.5 us), role constants formed in the reset block of one-step launches
//  (142 -> 128 VGPRs), observation rows carried out by the helper wave, per-episode action-map constants in the rollouts
//  (profiles/r04/ab_hoist_act.txt), Quad-v0's reward formed by the helper wave (§3.3 item 2; profiles/r03/ab_quad_builds.txt, q_norew),
//  a helper wave in qr_rollout_actor (§3.3 item 5: Coupled 65 536 envs, T = 32: 5.37 -> 4.51 us per env-step), the delta-form stages
//  of the rate-adaptive launches (numerics: tools/numerics_delta.py and the free-run rows of profiles/r03/parity_summary.txt, 6.8e-6
//  -> 2.4e-6; cost: the "free run in regime" rows of profiles/r03/runtime_ab.json, 4.39 against 4.03 us).  DESIGN.md /
//  docs/EXPERIMENTS.md name the files.)
constexpr unsigned kXcdGrid = 1536;  // one-step helper-wave launches up to this many tiles give every XCD a contiguous range of tiles (see tile_id)
// Grids up to this many tiles run the one-step kernel with a helper wave per tile (HELP).  The limit is an EMPIRICAL crossover,
// not a residency rule: 2560 tiles are 5120 waves, more than the 4096 wave slots the 120-VGPR kernel has at four waves per SIMD —
// the helper waves are short-lived and the launch still wins there (profiles/r03/ab_helper_thresholds.txt, with the write-through
// stores of DESIGN.md 3.5: Quad-v0 163 840 envs 7.3 against 8.3 us plain, 196 608 equal, 262 144 10.3 against 9.9).  Round 5, with
// the reward on the stepping wave beyond kHelpRewardTiles (one substep): 196 608 envs 8.0-8.2 against 8.8-8.9 plain, 229 376
// 8.6-9.2 against 9.7-9.8, 245 760 9.1-9.9 against 9.9-10.1, 262 144 9.8-10.6 against 10.1-10.3 (profiles/r05/ab_step_prio.txt):
// 3328 tiles for one substep; launches with more substeps keep 2560.  The environment variable QR_HELPER_GRID and the
// QR_FLAG_*_HELPER bits override it (see `tuning`).
constexpr unsigned kHelperGrid = 3328;
constexpr unsigned kHelperGridSubsteps = 2560;  // Quad-v0 with >= 2 substeps or the fused goal generator
constexpr unsigned kHelperGridRollout = 1024;   // qr_rollout / qr_rollout_actor (two waves per SIMD)
// The wrappers: ahead of the plain launch up to 262 144 envs while the action rows come
// from cache (r03/ab_helper_thresholds.txt, 8 slabs: 14.9 against 15.7 us), behind it beyond 131 072 envs when they stream from HBM (r03/ab_helper_wave.txt, 64 slabs:
// 131 072 envs 9.4 against 9.1 us, 262 144 envs 18.4 against 16.5 — three stepping waves per SIMD hide less latency than four).  Round 5, with the rows on
// the stepping wave beyond kHelpRowsTiles: ahead up to 163 840 envs with either action source (10.2-10.4 against 10.5-10.7), mixed at 196 608: 2560 tiles
// (one substep; 1664 with more: kHelperGridWrapSubsteps; 2048 with the fused goal generator)
constexpr unsigned kHelperGridWrap = 2560;
// ------------------------------------------------------------------------------------
// Quad-v0 reward and termination (quad.py:274-318) from the post-step state
// ------------------------------------------------------------------------------------
// reward_wrapper (quad.py:274-298), formed in float32 (its result is a float32 word)
template <typename T, typename X>
__device__ __forceinline__ float quad_reward_raw(const X (&x)[3], const X (&v)[3], const T (&q)[4], const T (&W)[3],
                                                 const float (&goal)[12], const Coeffs& c) {
  const T qw = q[0], qx = q[1], qy = q[2], qz = q[3];
  const T R00 = fma_1m2(fma_ss(qy, qy, qz, qz)), R10 = T(2) * fma_ss(qx, qy, qw, qz);  // b1 = first column of R(q)
  float eX2 = 0.f, eV2 = 0.f, W2 = 0.f;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float dx = (float)x[j] - goal[j], dv = (float)v[j] - goal[3 + j], wj = (float)W[j];
    eX2 = fmaf(dx, dx, eX2); eV2 = fmaf(dv, dv, eV2); W2 = fmaf(wj, wj, W2);
  }
  // eb1 = signed angle from b1d to b1_proj ~ (R00, R10, 0) (quad_utils.py:97-101,157-177).
  // acos(du.cu) with the sign of (du x cu)_z == atan2(|du x cu|, du.cu), which is invariant
  // to the lengths of both vectors, so neither is normalised.
  const float r00 = (float)R00, r10 = (float)R10;
  const float g6 = goal[6], g7 = goal[7], g8 = goal[8];
  const float dot = g6 * r00 + g7 * r10;
  const float cz = g6 * r10 - g7 * r00;
  const float hy2 = r00 * r00 + r10 * r10;
  const float sabs = sqrtf(g8 * g8 * hy2 + cz * cz);
  float ang = atan2_fast(sabs, dot);
  if (cz < 0.0f) ang = -ang;
  const float eb1 = ang * (float)(1.0 / kPi);
  return -c.Cx * eX2 - c.Cb1 * fabsf(eb1) - c.Cv * eV2 - c.CW * W2;
}

// done_wrapper (quad.py:301-318): roll = atan2(R21,R22), pitch = -asin(R20); |angle| >= 85 deg
// without inverse trig.  x, v: float32 numbers compared with the limit rounded UP to float32,
// which decides exactly as the float64 comparison does.  (bitwise | on purpose: no branches)
template <typename T, typename X>
__device__ __forceinline__ bool quad_done(const X (&x)[3], const X (&v)[3], const T (&q)[4], const T (&W)[3], const Coeffs& c) {
  const T qw = q[0], qx = q[1], qy = q[2], qz = q[3];
  const T R20 = T(2) * fma_sd(qx, qz, qw, qy), R21 = T(2) * fma_ss(qy, qz, qw, qx), R22 = fma_1m2(fma_ss(qx, qx, qy, qy));
  X xl, vl;
  if constexpr (std::is_same<X, float>::value) { xl = c.x_lim_up; vl = c.v_lim_up; } else { xl = X(c.x_lim); vl = X(c.v_lim); }
  bool d = false;
#pragma unroll
  for (int j = 0; j < 3; ++j)
    d = d | !(fabs(x[j]) < xl) | !(fabs(v[j]) < vl) | !(fabs(W[j]) < T(c.W_lim));
  d = d | !(fabs(R20) < T(c.sin_euler_lim));          // |pitch| >= lim
  d = d | !(fabs(R21) < T(c.tan_euler_lim) * R22);    // |atan2(R21,R22)| >= lim
  return d;
}

// The post-step state of a tile as its stepping wave leaves it in LDS for the helper wave (HELP, Quad-v0), which
// forms and stores the reward from it.
template <typename T, typename X>
struct PostLds {
  X x[3][64], v[3][64];
  T q[4][64], W[3][64];
  uint32_t done[64];  // the stepping wave's termination flag (the helper's crash override needs it: not formed twice)
};

// ------------------------------------------------------------------------------------
// The fused step / rollout kernel
// ------------------------------------------------------------------------------------
// TRAJ != 0 = the goal generator (utils/trajectory_generator.py) is fused into the step; separate instantiations
// so that the default path carries none of its registers: 1 = the stateless modes 0 / 1 / 6, 2 = the stateful modes 2-5
// (take-off, landing, stay, circle: persistent goal fields loaded / stored with the working set).  ADAPT = the
// rate-adaptive substep count (QrCoeffs::w_adapt); launch_kind() picks the plain instantiation
// whenever adaptivity provably cannot trigger.
// POLICY != 0 = qr_rollout_actor: the action of every step comes from the actor(s) evaluated on the
// env's current observation, which stays in registers from one step to the next.  1: PPO / TD3 actors
// (parameter log_std, tanh-of-mean rule); 2: any reference MLP actor (adds SAC's log_std head and rule).
// SINGLE = exactly one env-step per launch (qr_step): no loop over steps, so nothing is hoisted out of it and kept
// live across the whole kernel (fewer SGPRs to spill, a shorter prologue).
// HELP (with SINGLE, for grids in the launch-latency regime) = the workgroup carries a second wavefront that does
// nothing but sample the tile's reset pool into LDS while the stepping wave waits for its loads and integrates:
// a lone wave issues one VALU instruction per ~5.6 cycles, two waves on a SIMD one per ~2.9 (tools/valu_microbench.hip),
// so the helper runs in issue slots that are otherwise empty, and the stepping wave's reset block shrinks from
// ~230 instructions (Philox, role scaling, attitude, 24 cross-lane reads) to six LDS reads.
// MAG = the substeps are Magnus substeps (qr_dynamics.h: integrate_magnus; default layout, `substeps` >= 2 — the host's choice from
// the substep count alone, pick_instance); MAG = false kernels hold RK4 only and run the one-substep launches.
template <int KIND, typename XV, typename QW, int B, int TRAJ, bool ADAPT, int POLICY = 0, bool SINGLE = false, bool HELP = false, bool HREW = true,
          bool MAG = false>
__global__ __launch_bounds__(B + (HELP ? 64 : 0), ((HELP && POLICY) ? 2 : (TRAJ || POLICY) ? 1 : 2))  // (HELP: both waves of every tile resident)
void step_kernel(void* pos_vel, void* att_rate, const float* action, float* params, float* integ, int32_t* reset_count,
                 int32_t n_envs, int32_t ld_envs, const Args a_in) {
  // The leading scalar arguments duplicate the fields of Args that the wave's loads depend on: as
  // plain kernel arguments they are preloaded into SGPRs by the dispatcher (gfx950 kernarg
  // preload, -mllvm -amdgpu-kernarg-preload-count=16: 14 dwords is what the hardware hands over), so
  // every load of the working set — and the scalar load of the tile's reset counter — is issued in
  // the wave's first instructions, without waiting for a scalar-load round trip to the kernarg
  // segment (host-visible memory: ~0.7 us, measured with in-kernel clock stamps).
  // Everything else is read from the kernarg segment WHERE IT IS USED: referenced as a by-value
  // struct, every used field of Args would be loaded in the kernel's entry block (that is how the
  // AMDGPU backend lowers kernel arguments) and stay live in SGPRs from there on — far more than the
  // 102 a wave has, so the round-1 kernel spilled them into VGPR lanes (v_writelane / v_readlane, a
  // VALU slot each, ~220 on the step's path).  Through the segment pointer they are ordinary
  // scalar loads from constant memory with short live ranges.
#if defined(__HIP_DEVICE_COMPILE__)
  const Args& ka = *reinterpret_cast<const Args*>(reinterpret_cast<const char*>(__builtin_amdgcn_kernarg_segment_ptr()) + kArgsOffset);
  (void)a_in;
#else
  const Args& ka = a_in;  // (host pass of the single-source compile: never executed)
#endif
  QR_SPAN_BEGIN();
  Args a;  // the fields the helpers touch, assembled from the preloaded scalars
  a.pos_vel = pos_vel; a.att_rate = att_rate; a.action = action; a.params = params; a.integ = integ;
  a.reset_count = reset_count;
  a.n = n_envs; a.ld = ld_envs;
  using T = QW;  // q, W are held and accumulated in their storage type
  using X = XV;  // and so are x, v
  using KT = KindTraits<KIND>;
  constexpr int A = KT::A, D0 = KT::D0, D1 = KT::D1 ? KT::D1 : 1, NAG = KT::NAG;
  constexpr int AUX = (HELP && SINGLE) ? kHelpAux : kPlainAux;  // cache policy of every store of this launch (qr_args.h)
  __shared__ __attribute__((aligned(16))) float smem[B * (D0 > A ? D0 : A)];
  const int tid = threadIdx.x;
  const unsigned lane = threadIdx.x;
  // XCD-aware tile map.  Workgroups are dealt round-robin over the 8 XCDs (workgroup b runs on XCD b % 8).  With tile = blockIdx.x
  // an XCD therefore touches every EIGHTH 256- / 512-byte segment of each SoA field — its requests alias onto a few of its L2's
  // channels.  For the grids whose working set is cache-resident (the one-step helper-wave launches up to kXcdGrid tiles) every XCD
  // gets a CONTIGUOUS range of tiles instead (a bijection for any tile count: XCD x owns q + (x < r) tiles, q = tiles / 8, r = tiles % 8):
  // 16 384 ... 81 920 envs 0.5-4 % faster for all three kinds (Quad-v0 65 536: 4.15 -> 4.07 us, Coupled 5.34 -> 5.18, Decoupled 5.17 ->
  // 4.98; profiles/r05/ab_xcd_map.txt), nothing at <= 8192 envs.  Larger grids stream from HBM, where the default deal keeps the eight
  // XCDs inside the same DRAM pages: kept there (1 M envs: +1.7 % with contiguous ranges).  Which workgroup steps which tile changes no
  // result bit (tools/ab_equal.py: identical).
  unsigned tile_id = blockIdx.x;
  if constexpr (HELP && SINGLE) {
    const unsigned n_tiles = ((unsigned)n_envs + 63u) >> 6;
    if (n_tiles <= kXcdGrid) {
      const unsigned xcd = blockIdx.x & 7u, q8 = n_tiles >> 3, r8 = n_tiles & 7u;
      tile_id = xcd * q8 + (xcd < r8 ? xcd : r8) + (blockIdx.x >> 3);
    }
  }
  if constexpr (HELP && !SINGLE) tile_id += (unsigned)ka.tile_base;  // (a chunk of a larger grid: launch_kind)
  const unsigned ufirst = tile_id * (unsigned)B;
  const int64_t first = (int64_t)ufirst;
  const int64_t i = first + tid;
  const int64_t N = a.n, L = a.ld;
  const int rows = min(n_envs - (int)ufirst, B);   // (n_envs < 2^31: checked on the host)
  const bool active = tid < rows;
  // lanes past a ragged tail read the tail's last env (valid memory, finite numbers) and store nothing
  const unsigned ll = min(lane, (unsigned)(rows - 1));
  // (Measured and NOT adopted, profiles/r03/ab_dev_coeffs.txt: the coefficient block in a device-resident global instead of
  // the kernarg segment — 4.63 against 4.16 us per launch at 65 536 envs.)
  const Coeffs& c = ka.c;
  static_assert(!HELP || B == 64, "the helper wave belongs to the one-wave-per-tile kernels");
  // (a rollout alternates between two pools: the helper samples step t+1's while the stepping wave takes from step t's)
  __shared__ typename std::conditional<HELP, PoolLds<T>, char>::type pool_lds[(SINGLE || POLICY) ? 1 : 2];  // (unused without HELP: dropped)
  // (POLICY with a helper wave) the step's exploration noise, sampled a step ahead by the helper: [t & 1][lane][8]
  __shared__ __attribute__((aligned(16))) float eps_lds[HELP && POLICY ? 2 * 64 * 8 : 4];
  // Quad-v0's reward (an atan2, a sqrt: ~90 instructions) is formed by the helper wave as well
  // (HREW = false: the one-step Quad-v0 launch on grids where some SIMDs hold a second stepping wave — launch_kind)
  constexpr bool kHelpReward = HELP && !POLICY && !TRAJ && KIND == QR_KIND_QUAD && HREW;  // (TRAJ: the goal lives in the stepping wave's registers)
  __shared__ typename std::conditional<kHelpReward, PostLds<T, X>, char>::type post_lds[SINGLE ? 1 : 2];  // (a rollout alternates)
  __shared__ PoolLds<T> own_pool;  // pools this wave samples itself (no helper; or a tile's 13th.. resetting lane)
  // (HREW = false for a wrapper: the rows stay with the stepping wave — one-step grids beyond kHelpRowsTiles tiles, launch_kind)
  constexpr bool kHelpRows = HELP && SINGLE && (KIND == QR_KIND_QUAD || HREW);
  // (plain one-step wrapper kernels: large grids) the observation rows go to their LDS tile as soon as they are formed,
  // BEFORE the reset block, and a re-sampled env overwrites its row there: the 18-23 row registers need not survive the
  // reset block.  With the late loads below: Coupled 150 -> 114 VGPRs, Decoupled 148 -> 115, i.e. four waves per SIMD
  // (262 144 envs 19.1 -> 16.5 us).  Not in the helper-wave launches, where the second write of a re-sampled env's row
  // is on the stepping wave's path (65 536 envs: 6.03 -> 6.15 us with it).
  constexpr bool kEarlyTile = SINGLE && !HELP && !POLICY && KIND != QR_KIND_QUAD;
  __shared__ __attribute__((aligned(16))) float smem1[(kHelpRows || kEarlyTile || (HELP && POLICY)) && KT::D1 > 0 ? B * D1 : 4];  // (Decoupled: both tiles at once)
  // (rollouts of the wrappers with a helper wave) the observation rows of step t go to tile t & 1 at the end of the step and the
  // helper carries them out behind the next step's pool barrier: 91 vector instructions and 24 stores per env-step off the
  // stepping wave (65 536 envs, T = 100: Coupled and Decoupled 2.14 -> 1.89 us per env-step; identical bits; profiles/r05/ab_roll_rows.txt)
  constexpr bool kRollRows = HELP && !SINGLE && !POLICY && KIND != QR_KIND_QUAD;
  __shared__ __attribute__((aligned(16))) float rtile0[kRollRows ? 2 * B * D0 : 4];
  __shared__ __attribute__((aligned(16))) float rtile1[kRollRows && KT::D1 > 0 ? 2 * B * D1 : 4];
  if constexpr (HELP) {
    // (the wave's first lane decides: a wave-uniform branch in the compiler's eyes too — on threadIdx.x itself everything
    // after it counts as divergent control flow, and scalar offsets of the loads below were re-derived per lane)
    if (__builtin_amdgcn_readfirstlane((int)threadIdx.x) >= B) {  // ---- the helper wavefront: pass 0 of the tile's reset pool -> LDS ----  //@sec helper-wave
      float hgoal[12];
      hover_goal(hgoal);
      if constexpr (kHelpReward) {
        if (float* const gp = ka.goal) {
          const SoA<float> goal(gp, 12, ld_envs);
          const unsigned hll = min(threadIdx.x - B, (unsigned)(rows - 1));
#pragma unroll
          for (int f = 0; f < 9; ++f) hgoal[f] = goal.load(f, ufirst, hll);
        }
      }
      // the helper's own output pointers, read with its first scalar loads: behind the barriers they would be a kernarg
      // cache miss at the very end of the launch
      float* const hob0 = ka.obs0;
      float* const hob1 = KT::D1 > 0 ? ka.obs1 : nullptr;
      float* const hrew = ka.reward;
      float* const hraw = ka.reward_raw;
      asm volatile("" ::"s"(hob0), "s"(hob1), "s"(hrew), "s"(hraw));
      const uint32_t rc = (uint32_t)reset_count[tile_id];
      const uint32_t hflags = ka.flags;
      const uint64_t hseed = ka.seed;
      const uint64_t hgfirst = (uint64_t)(ka.env_offset + first);
      // (Measured and NOT adopted, profiles/r03/ab_helper_touch.txt: requesting this wave's kernarg lines with dummy loads in its
      // first instructions, like the stepping wave does — 4.148 against 4.151 us per launch; the pool is in LDS ~0.7 us before
      // the stepping wave asks for it either way.)
      const bool heval = (hflags & QR_FLAG_EVAL_RESET) != 0;
      PoolRole hrole;
      pool_role(hrole, !heval && !(hflags & QR_FLAG_NO_UDM) && params != nullptr, heval, c);
      // the reward of env-step t from the post-step state the stepping wave left in LDS (kHelpReward)
      auto help_reward = [&](int t) {
        if constexpr (kHelpReward) {
          const unsigned hl = threadIdx.x - B;
          const auto& ps = post_lds[SINGLE ? 0 : (t & 1)];
          X hx[3], hv[3];
          T hq[4], hW[3];
#pragma unroll
          for (int j = 0; j < 3; ++j) { hx[j] = ps.x[j][hl]; hv[j] = ps.v[j][hl]; hW[j] = ps.W[j][hl]; }
#pragma unroll
          for (int j = 0; j < 4; ++j) hq[j] = ps.q[j][hl];
          const float r = quad_reward_raw<T, X>(hx, hv, hq, hW, hgoal, c);
          // (rollouts: the stepping wave's own flag — the helper there is about as long as the stepping wave, 1.297 -> 1.283 us per
          //  env-step without the second quad_done; one-step launches: formed here, 4.13 against 4.16 us with the LDS word)
          const bool d = SINGLE ? quad_done<T, X>(hx, hv, hq, hW, c) : (ps.done[hl] != 0u);
          if ((int)hl < rows) {
            const int64_t hrow = (int64_t)t * n_envs + first;
            gstore<AUX>(hrew + hrow + hl, d ? -1.0f : interp01(r, c.rmin_mono, c.inv_nrmin_mono));  // crash override (quad.py:162-166)
            if (hraw) gstore<AUX>(hraw + hrow + hl, r);
          }
        }
      };
      ResetPool<T> hp;
      if constexpr (POLICY != 0) {
        // qr_rollout_actor.  Per env-step t the helper meets the stepping wave twice: B1(t), at the top of the step — the
        // step's noise is in LDS and the tile holds the observation rows of step t-1 (which this wave then carries out while
        // the stepping wave evaluates the actor) — and B2(t), when the step's reset pool and the NEXT step's noise are in LDS.
        const int hsteps = ka.n_steps;
        const int hl = (int)threadIdx.x - B;
        const bool own_noise = !ka.deterministic && ka.noise == nullptr;
        const uint64_t nseed = ka.noise_seed, sbase = ka.step_base, hgid = (uint64_t)(ka.env_offset + first + hl);
        float* const ob0 = hob0;
        float* const ob1 = hob1;
        auto make_eps = [&](int t) {
          if (!own_noise) return;
          float z[4];
          normal4(z, nseed, hgid, sbase + (uint64_t)t, 0u);
          float* e = eps_lds + ((t & 1) * 64 + hl) * 8;
          *reinterpret_cast<float4*>(e) = make_float4(z[0], z[1], z[2], z[3]);
          if constexpr (A > 4) {
            normal4(z, nseed, hgid, sbase + (uint64_t)t, 1u);
            e[4] = z[0];
          }
        };
        make_eps(0);
        for (int t = 0; t < hsteps; ++t) {
          asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // B1(t)
          if (t > 0) {
            lds_to_rows<B, D0, AUX>(ob0 + ((int64_t)(t - 1) * n_envs + first) * D0, smem, hl, rows);
            if constexpr (KT::D1 > 0) lds_to_rows<B, D1, AUX>(ob1 + ((int64_t)(t - 1) * n_envs + first) * D1, smem1, hl, rows);
          }
          make_pool<T>(hp, hrole, hseed, hgfirst, rc + (uint32_t)t, 0);
          pool_to_lds(pool_lds[0], hp);
          if (t + 1 < hsteps) make_eps(t + 1);
          asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // B2(t)
        }
        asm volatile("s_barrier" ::: "memory");  // the tile of the last step
        lds_to_rows<B, D0, AUX>(ob0 + ((int64_t)(hsteps - 1) * n_envs + first) * D0, smem, hl, rows);
        if constexpr (KT::D1 > 0) lds_to_rows<B, D1, AUX>(ob1 + ((int64_t)(hsteps - 1) * n_envs + first) * D1, smem1, hl, rows);
        QR_SPAN_END();
        return;
      }
      if constexpr (!SINGLE) {  // a rollout: one pool per env-step, each handed over at that step's barrier
        const int hsteps = ka.n_steps;
        for (int t = 0; t < hsteps; ++t) {
          make_pool<T>(hp, hrole, hseed, hgfirst, rc + (uint32_t)t, 0);
          pool_to_lds(pool_lds[t & 1], hp);
          asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
          help_reward(t);  // (Quad-v0) this step's reward, before the next step's pool
          if constexpr (kRollRows) {  // (wrappers) the rows of step t - 1: complete in their tile since the end of that step
            if (t > 0) {
              const int hl = (int)threadIdx.x - B;
              lds_to_rows<B, D0, AUX>(hob0 + ((int64_t)(t - 1) * n_envs + first) * D0, rtile0 + ((t - 1) & 1) * (B * D0), hl, rows);
              if constexpr (KT::D1 > 0) lds_to_rows<B, D1, AUX>(hob1 + ((int64_t)(t - 1) * n_envs + first) * D1, rtile1 + ((t - 1) & 1) * (B * D1), hl, rows);
            }
          }
        }
        if constexpr (kRollRows) {  // the last step's rows
          asm volatile("s_barrier" ::: "memory");
          const int hl = (int)threadIdx.x - B;
          lds_to_rows<B, D0, AUX>(hob0 + ((int64_t)(hsteps - 1) * n_envs + first) * D0, rtile0 + ((hsteps - 1) & 1) * (B * D0), hl, rows);
          if constexpr (KT::D1 > 0) lds_to_rows<B, D1, AUX>(hob1 + ((int64_t)(hsteps - 1) * n_envs + first) * D1, rtile1 + ((hsteps - 1) & 1) * (B * D1), hl, rows);
        }
        QR_SPAN_END();
        return;
      }
      make_pool<T>(hp, hrole, hseed, hgfirst, rc, 0);
      pool_to_lds(pool_lds[0], hp);
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      if constexpr (kHelpReward) help_reward(0);  // ---- then the reward of the step, from the post-step state the stepping wave left in LDS ----
      if constexpr (kHelpRows) {  // ---- and the observation rows: the stepping wave leaves the tile in LDS, this wave carries it out ----
        if (KIND != QR_KIND_QUAD || hob0 != nullptr) {
          asm volatile("s_barrier" ::: "memory");
          const int hl = (int)threadIdx.x - B;
          lds_to_rows<B, D0, AUX>(hob0 + first * D0, smem, hl, rows);
          if constexpr (KT::D1 > 0) lds_to_rows<B, D1, AUX>(hob1 + first * D1, smem1, hl, rows);
        }
      }
      QR_SPAN_END();
      return;
    }
  }
  // Issue priority of the stepping wave over the helper wave it shares a SIMD with (and over its own helper in the CU's shared
  // front end): the helper then runs in the slots the stepping wave leaves empty instead of taking every other one.  Multi-step
  // launches: for the whole launch — the helper's work per step is a third of the stepping wave's and is asked for a step later
  // (65 536 envs, per env-step: Quad-v0 rollout 1.44 -> 1.29 us, Coupled 2.25 -> 2.12, PPO collection step 3.55 -> 3.17).
  // One-step launches: the helper's pool is wanted within the same microsecond and its reward / rows trail the launch, so only
  // up to the pool barrier and only on grids of at most 768 tiles (32 768 envs: wrappers -3.7 %, Quad-v0 -1.5 %; 65 536 envs
  // +0.3...3 %, 98 304 +9 % with it).  Changes no result.  profiles/r05/ab_step_prio.txt
  if constexpr (HELP && !SINGLE) __builtin_amdgcn_s_setprio(kStepPrio);
  if constexpr (HELP && SINGLE) {
    if ((((unsigned)n_envs + 63u) >> 6) <= kPrioSingleTiles) __builtin_amdgcn_s_setprio(kStepPrio);
  }
  //@sec prologue-loads
#if defined(__HIP_DEVICE_COMPILE__)
  // The coefficient block spans five 64-byte lines of the kernarg segment (host-visible memory: ~0.5 us per miss).  The
  // compiler reads coefficients where they are used, i.e. it requests those lines only AFTER the first batch of scalar
  // loads is back, and the first arithmetic then waits for them.  One dummy word per line, requested with the wave's
  // first instructions, has them in the scalar cache by then.  (The words are never used; their registers stay
  // reserved until a point behind the first scalar wait, see below.)
  uint32_t ctouch[6];  // ([5]: the line of the per-call integers — substeps is wanted at the first RK4 stage)
  {
    constexpr int kC = kArgsOffset + (int)offsetof(Args, c);
    asm volatile("s_load_dword %0, %6, %7\n\ts_load_dword %1, %6, %8\n\ts_load_dword %2, %6, %9\n\t"
                 "s_load_dword %3, %6, %10\n\ts_load_dword %4, %6, %11\n\ts_load_dword %5, %6, %12"
                 : "=&s"(ctouch[0]), "=&s"(ctouch[1]), "=&s"(ctouch[2]), "=&s"(ctouch[3]), "=&s"(ctouch[4]), "=&s"(ctouch[5])
                 : "s"(__builtin_amdgcn_kernarg_segment_ptr()), "i"(kC), "i"(kC + 64), "i"(kC + 128), "i"(kC + 192), "i"(kC + 256),
                   "i"(kArgsOffset + (int)offsetof(Args, substeps)));
  }
#endif

  // ---- issue the loads of the env's working set (SoA, lane-contiguous) and of its action row ----
  Work<T, X> w;
  float act_next[A];
#pragma unroll
  for (int j = 0; j < A; ++j) act_next[j] = 0.f;
  // Action rows [N][A] -> lane registers (load_action_row).  In a rollout
  // the row of step t+1 is requested before the arithmetic of step t, so its latency is hidden.
  const bool auto_reset = HELP || reset_count != nullptr;  // passed only with QR_FLAG_AUTO_RESET: its presence IS the flag, known without a load
  PoolRole role;
  uint32_t rcount_s = 0;  // the tile's position in the in-launch reset stream
  // (Measured and NOT adopted, profiles/r03/ab_load_order_store_policy.txt: requesting parameters and action row first, x and v
  // last, and rebuilding the quaternion behind the action map — 4.47 against 4.46 us per launch at 65 536 envs.)
  // (kHeadOrder) The one-step helper-wave launches: one stepping wave per SIMD, nothing overlaps its instruction stream, and a
  // wave's loads land in issue order over several hundred nanoseconds (load_state_raw).  There the queue is ordered by FIRST USE —
  // packed attitude, parameters, action row, rates, x and v (wanted only by the step's final update) — and the head of the step
  // is pinned in the same order (sched_barrier below): the attitude unpack, the per-launch step size, the action-map constants and
  // the action map each run behind a partial vmcnt wait while the words behind them are still in flight, instead of behind the
  // wait for the whole working set.  The arithmetic is the same instructions on the same operands: no result bit moves.
  // 65 536 envs, Quad-v0: 4.12 -> 3.82 us per launch; the queue's order alone 3.88, the pins alone 4.06 (profiles/r25/ab_head.txt).
  // Not the instantiations of the larger grids, where SIMDs hold a second stepping wave and a wave's wait is another wave's time
  // (HREW = false; MAG, the launches with two or more substeps: 131 072 envs x 10 substeps 6.66 -> 6.80 us with it).
  constexpr bool kHeadOrder = HELP && SINGLE && !POLICY && !TRAJ && HREW && !MAG;
  QuatPack<T> qin;
  if constexpr (kHeadOrder) { load_att_packed<QW>(a, ufirst, ll, qin); __builtin_amdgcn_sched_barrier(0); }
  else load_state<XV, QW>(a, first, ll, w);
  w.nominal = a.params == nullptr;
  {  // (without a params buffer: a descriptor without records, the loads return 0 — no branch between the load batches)
    const SoA<float> prm(a.params, 6, L);
#pragma unroll
    for (int f = 0; f < 6; ++f) w.prm[f] = prm.load(f, ufirst, ll);
  }
  if constexpr (kHeadOrder) __builtin_amdgcn_sched_barrier(0);  // (the queue's order is the point: no clustering across the groups)
  if constexpr (!POLICY) load_action_row(a.action + first * A, ll, act_next);
  if constexpr (kHeadOrder) { __builtin_amdgcn_sched_barrier(0); load_rate_pos_vel<XV, QW>(a, ufirst, ll, w); }
  // The tile's position in the in-launch reset stream: a scalar load.  (Measured alternatives, bench.py at 65 536 envs:
  // a vector load at the end of the wave's load queue 5.71 us, at its front 5.70 us, a load deferred until the working set
  // has been consumed 6.12 us — against 5.42 us, although scalar loads return out of order and the first use of a kernarg
  // coefficient therefore also waits for this one: the in-kernel timelines of those variants are shorter, their launches not.)
  if (!HELP && auto_reset) rcount_s = (uint32_t)reset_count[tile_id];
  // (kLateLoads) The plain one-step wrapper kernel serves grids of several waves per SIMD, where a load's latency is
  // other waves' time: it requests the 20 words only the error observation wants (goal, integrators) AFTER the
  // integration instead of holding them across it — registers for occupancy.
  constexpr bool kLateLoads = SINGLE && !HELP && !ADAPT && !TRAJ && !POLICY && KIND != QR_KIND_QUAD;
  if constexpr (KIND != QR_KIND_QUAD && !kLateLoads) {
    const SoA<float> integ(a.integ, 8, L);
#pragma unroll
    for (int f = 0; f < 8; ++f) w.integ[f] = integ.load(f, ufirst, ll);
  } else {
#pragma unroll
    for (int f = 0; f < 8; ++f) w.integ[f] = 0.0f;
  }
  // ---- the rest of the arguments: one batch of scalar loads from the kernarg segment ----  //@sec prologue-args
  const uint32_t flags = ka.flags;
  const uint64_t seed = ka.seed;
  const uint64_t gfirst = (uint64_t)(ka.env_offset + first);
  float* const goal_ptr = ka.goal;
  int32_t* const steps_ptr = ka.steps;
  const int n_steps = SINGLE ? 1 : ka.n_steps;
  const bool eval_reset = (flags & QR_FLAG_EVAL_RESET) != 0;
  const bool randomise = !eval_reset && !(flags & QR_FLAG_NO_UDM) && a.params != nullptr;
  // One-step launches form the role constants in the reset block (below); a rollout forms them once, here.
  constexpr bool kLazyRole = SINGLE;
  if (!kLazyRole && !HELP && auto_reset) pool_role(role, randomise, eval_reset, c);  // (scalars only: runs while the loads are in flight)
#pragma unroll
  for (int f = 0; f < 12; ++f) w.goal[f] = f == 6 ? 1.0f : 0.0f;  // hover default (quad.py:98-101; written out, not hover_goal: docs/EXPERIMENTS.md "refactor")
  if (!TRAJ && !kLateLoads && goal_ptr) {  // (with the fused generator the goal is formed in registers every step)
    const SoA<float> goal(goal_ptr, 12, L);
#pragma unroll
    for (int f = 0; f < 12; ++f) w.goal[f] = goal.load(f, ufirst, ll);
  }

  // ---- in-launch reset: this wave's pool of episode starts (qr_rng.h), sampled while the loads are in flight ----
  // (Measured and NOT adopted, profiles/r02/ab_quad_builds.txt, columns q_spec / q_nohelp: sampling the pool speculatively in the
  // same wave right after issuing its loads — 5.86-5.92 against 5.28 us per launch at 65 536 envs: the pool's inputs arrive only
  // ~0.5 us after the wave's first instruction, so most of its ~0.6 us does not hide under the loads and EVERY wave pays it.)
  ResetPool<T> pool;

  Traj tr;
  const int goal_mode = TRAJ ? ka.goal_mode : QR_GOAL_EXTERNAL;  // wave-uniform
  constexpr bool kStateful = TRAJ == 2;
  if constexpr (TRAJ) {
    const SoA<float> traj(ka.traj, 8, L);
#pragma unroll
    for (int f = 0; f < (kStateful ? 8 : 7); ++f) tr.set(f, traj.load(f, ufirst, ll));
    if constexpr (kStateful) {  // xd, vd, b1d, Wd persist in the goal buffer (required for these modes)
      const SoA<float> goal(goal_ptr, 12, L);
#pragma unroll
      for (int f = 0; f < 12; ++f) w.goal[f] = goal.load(f, ufirst, ll);
    }
  }
#if defined(__HIP_DEVICE_COMPILE__)
  // (steps_ptr is back => s_waitcnt lgkmcnt(0) has been passed => the dummy words have landed: their registers are free)
  asm volatile("" ::"s"(ctouch[0]), "s"(ctouch[1]), "s"(ctouch[2]), "s"(ctouch[3]), "s"(ctouch[4]), "s"(ctouch[5]), "s"(steps_ptr));
#endif
  int32_t steps = (steps_ptr && active) ? (steps_ptr + first)[lane] : 0;
  bool params_dirty = false;
  bool traj_dirty = false;  // this lane started a new episode: its generator state changed
  bool stored_early = false;  // (SINGLE) this lane's state went out before its wave sampled a reset pool
  // (n_envs: a preloaded SGPR — gridDim.x would be a scalar load.  With a helper wave the reset block is six LDS reads:
  // nothing to overlap.)
  const bool early_store = SINGLE && !HELP && n_envs <= kEarlyStoreGrid * 64;
  QuatPack<T> qp;             // attitude in its storage form, formed once per env-step
  qp.k[0] = qp.k[1] = qp.k[2] = T(0);

  //@sec prologue-policy
  // POLICY: the observation the next action is computed from (rows -> lane registers once, then
  // carried from step to step)
  float po0[D0], po1[D1];
  // agent 0 (23 / 15 -> 16 -> 16 -> 4, args_parse.py:40, main.py:68-73) on the matrix cores, weights
  // resident in registers; agent 1 of DECOUPLED (3 -> 4 -> 4 -> 1: 32 FMAs) per lane from LDS
  constexpr bool GENERAL = POLICY == 2;
  ActorMfma<D0, GENERAL> actor0;
  using Actor1 = ActorLds<3, 4, 1>;
  __shared__ __attribute__((aligned(16))) float wsm[POLICY ? Actor1::SIZE : 4];
  if constexpr (POLICY) {
    load_rows<B, D0>(ka.obs0_in + first * D0, po0, smem, tid, rows);
    if constexpr (KT::D1 > 0) load_rows<B, D1>(ka.obs1_in + first * D1, po1, smem, tid, rows);
    actor0.load(ka.actor[0], tid);
    if constexpr (KT::D1 > 0) Actor1::fill(wsm, ka.actor[1], tid);
    // (HELP) the tile always holds the current observation rows: written here and at the end of every step, read by the
    // first layer's MFMAs and — as the rows of the step that produced them — carried out by the helper wave
    if constexpr (HELP) rows_to_lds<D0>(po0, smem, tid);
    tile_sync<B>();
  }

  // What the action map needs of the PARAMETERS only (masses, inertias, their reciprocals: qr_dynamics.h, ActConsts) changes only
  // when an env is re-sampled: a rollout forms it here and again behind a reset, not in every env-step.  (Not with the policy in
  // the loop: those kernels are at their register limit; not for Decoupled, whose rollout kernel is 1 % SLOWER with the 22 more
  // registers held across the loop.  Measured, profiles/r04/ab_hoist_act.txt: Quad-v0 65 536 envs 1.492 -> 1.469 us per env-step,
  // 262 144 envs 4.515 -> 4.354 = 60.2 G env-steps/s; Coupled 2.321 -> 2.289.)
  constexpr bool kHoistAct = !SINGLE && !POLICY && KIND != QR_KIND_DECOUPLED;
  // (Measured and NOT adopted, profiles/r05/ab_rollout_diet.txt: the same constants parked in LDS by the kernels that cannot afford the
  // registers — bit-identical, qr_rollout_actor 0.3-1.5 % and the Decoupled rollout 5 % SLOWER: eight ds_read_b64 on a lone wave's
  // critical path cost more than the ~30 VALU instructions they replace.)
  ActConsts<T> ac;
  if constexpr (kHoistAct) act_consts(w, c, ac);

  //@sec head-unpack
  // (kHeadOrder) the substep size is the same number in every lane and needs only scalars: its reciprocal chain (v_rcp_f64 and two
  // Newton steps, all dependent) is formed HERE, in the load wait; then the attitude, behind the wait for its three words alone
  T hstep = T(0);
  if constexpr (kHeadOrder) {
    if constexpr (!ADAPT) {
      hstep = T(c.dt) * recip(T(ka.substeps));
      asm volatile("" : "+v"(hstep));
    }
    unpack_quat(qin, w.q);
    {
      // (ordinary arithmetic floats across a sched_barrier before instruction selection: the values themselves are pinned — the
      // quaternion is complete at this statement, and the parameter words are first looked at behind it)
      asm volatile("" : "+v"(w.q[0]), "+v"(w.q[1]), "+v"(w.q[2]), "+v"(w.q[3]));
      asm volatile("" : "+v"(w.prm[0]), "+v"(w.prm[1]), "+v"(w.prm[2]), "+v"(w.prm[3]), "+v"(w.prm[4]), "+v"(w.prm[5]));
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  for (int t = 0; t < n_steps; ++t) {  //@sec action-source
    float act[A];
    if constexpr (POLICY) {
      float pre[A], ls[A], eps[A], logp[A];
      // the wave's observation rows -> LDS tile [lane][D0] (B operands of the first layer)
      if constexpr (!HELP) {
#pragma unroll
        for (int j = 0; j < D0; ++j) smem[tid * D0 + j] = po0[j];
        tile_sync<B>();
      }
      // B1(t), BEFORE the heads: the tile already holds the rows of step t - 1 (written at the end of that step) and the step's
      // noise was sampled before B2(t - 1), so the helper carries the rows out and samples the step's pool and the next step's
      // noise while this wave waits on the matrix pipe — in slots that are empty.  (Behind the heads, as before round 5, the
      // helper's work was the critical section between B1 and B2: Decoupled PPO collection 4.16 -> 3.43 us per env-step, SAC forms
      // -5...7 %, Coupled PPO -1.4 %; identical bits.  profiles/r05/ab_b1_early.txt)
      if constexpr (HELP) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      {
        float p0[4], l0[4];
        actor0.heads(smem, tid, p0, l0);
#pragma unroll
        for (int j = 0; j < 4; ++j) { pre[j] = p0[j]; ls[j] = l0[j]; }
      }
      if constexpr (KIND == QR_KIND_DECOUPLED) {
        float p1[1], l1[1];
        Actor1::heads(wsm, GENERAL && ka.actor[1].ls_w != nullptr, po1, p1, l1);
        pre[A - 1] = p1[0]; ls[A - 1] = l1[0];
      }
#pragma unroll
      for (int j = 0; j < A; ++j) eps[j] = 0.0f;
      if (!ka.deterministic) {
        if (ka.noise != nullptr) {  // injected draws [T][N][A]
          if (active) {
            const float* nbase = ka.noise + ((int64_t)t * N + first) * A;
#pragma unroll
            for (int j = 0; j < A; ++j) eps[j] = nbase[lane * A + j];
          }
        } else if constexpr (HELP) {  // sampled by the helper wave, one step ahead
          const float* e = eps_lds + ((t & 1) * 64 + tid) * 8;
          const float4 z4 = *reinterpret_cast<const float4*>(e);
          eps[0] = z4.x; eps[1] = z4.y; eps[2] = z4.z; eps[3] = z4.w;
          if constexpr (A > 4) eps[A - 1] = e[4];
        } else {
          float z[4];
          normal4(z, ka.noise_seed, (uint64_t)(ka.env_offset + i), ka.step_base + (uint64_t)t, 0u);
#pragma unroll
          for (int j = 0; j < 4; ++j) eps[j] = z[j];
          if constexpr (A > 4) {
            normal4(z, ka.noise_seed, (uint64_t)(ka.env_offset + i), ka.step_base + (uint64_t)t, 1u);
            eps[A - 1] = z[0];
          }
        }
      }
      if constexpr (!HELP) tile_sync<B>();  // the tile is reused by the row stores below
      actor_sample<4, GENERAL>(ka.actor[0].squash, actor0.ls_head, &pre[0], &ls[0], &eps[0], ka.deterministic != 0, ka.max_action, &act[0], &logp[0]);
      if constexpr (A > 4)
        actor_sample<1, GENERAL>(ka.actor[1].squash, ka.actor[1].ls_w != nullptr, &pre[A - 1], &ls[A - 1], &eps[A - 1], ka.deterministic != 0,
                        ka.max_action, &act[A - 1], &logp[A - 1]);
      if (active) {
        const int64_t arow = ((int64_t)t * N + first) * A;
        if constexpr (A == 4) {
          gstore<AUX>(reinterpret_cast<float4*>(ka.act_out + arow) + lane, make_float4(act[0], act[1], act[2], act[3]));
          if (ka.logp_out) gstore<AUX>(reinterpret_cast<float4*>(ka.logp_out + arow) + lane, make_float4(logp[0], logp[1], logp[2], logp[3]));
        } else {
#pragma unroll
          for (int j = 0; j < A; ++j) {
            gstore<AUX>(ka.act_out + arow + lane * A + j, act[j]);
            if (ka.logp_out) gstore<AUX>(ka.logp_out + arow + lane * A + j, logp[j]);
          }
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < A; ++j) act[j] = act_next[j];
      if (t + 1 < n_steps) load_action_row(a.action + ((int64_t)(t + 1) * N + first) * A, ll, act_next);
    }

    // ---- goal for this step from the pre-step state (main.py:145-147) ----  //@sec traj-goal
    if constexpr (TRAJ) {
      float b1d_dot[3];
      traj_goal<kStateful>(w, tr, goal_mode, c, b1d_dot);
    }
    // ---- action_wrapper ----  //@sec action-map
    Dyn<T> dyn;
    if constexpr (!kHoistAct) act_consts(w, c, ac);
    if constexpr (kHeadOrder) __builtin_amdgcn_sched_barrier(0);  // (the constants need the parameter words only, the map the action row: see kHeadOrder)
    action_map<KIND, T, X>(act, w, ac, c, dyn);
    if constexpr (kHeadOrder) __builtin_amdgcn_sched_barrier(0);
    if constexpr (SINGLE && !HELP) {  // (plain one-step launch: the loaded parameters are dead from here on — a re-sampled
#pragma unroll                        //  env stores the ones it takes from the pool — so their registers need not survive)
      for (int f = 0; f < 6; ++f) w.prm[f] = 0.0f;
    }
    // The output pointers sit in a kernarg cache line that nothing before the epilogue touches.  In the plain
    // instantiation (large grids) they are read with the first batch of scalar loads, so that the scalar-cache miss does
    // not sit in front of the first output store with the wave's registers held meanwhile (1 M envs: Quad-v0 36.6 -> 34.0 us,
    // Coupled 62.8 -> 59.5).  In the helper-wave launches — one stepping wave per SIMD, every wait on its critical path —
    // that batch is the wave's first wait and the extra line lengthens it: there they are read where they are used
    // (65 536 envs: 4.41 us against 4.49 with the early read, 4.67 with a read pinned behind the action map).
    uint8_t* const done_ptr = ka.done;
    uint8_t* const trunc_ptr = ka.truncated;
    if constexpr (!HELP) asm volatile("" ::"s"(done_ptr), "s"(trunc_ptr));
    // ---- observation_wrapper: integrate over dt with zero-order-hold (f, M) ----  //@sec integrate
    // The reference's DOP853 is adaptive (6 % of its steps subdivide); the fixed-step stand-in
    // is made rate-adaptive: RK4's local error grows like (|W| h)^5, so a wave that contains an
    // env spinning faster than w_adapt takes ceil(max|W_i| / w_adapt) times the substeps.  The
    // multiplier is the wave's maximum (found with ballots, so the substep loop stays wave-uniform
    // and in regime — |W| < 2 pi < w_adapt — this costs one ballot): every lane takes at least
    // the count its own rate asks for.
    if constexpr (ADAPT) {
      // (kDelta) The launches that step envs on without in-launch resets — in which an env can leave the regime — and those
      // with resets whose W_lim puts the re-sampling bound within reach of w_adapt (wants_adapt: 2.5 W_lim > w_adapt) form the quaternion stages in delta form (qr_dynamics.h: integrate_delta): their free run lands on RK4's
      // truncation floor instead of 7x above it.  qr_rollout_actor keeps the plain stages (its kernel is at its register limit).
      constexpr bool kDelta = !POLICY;
      const T wmax = fmax(fmax(fabs(w.W[0]), fabs(w.W[1])), fabs(w.W[2]));
      const T need = wmax * T(c.inv_w_adapt);
      if constexpr (kDelta) {
        int mul = 1;
        if (__ballot(need > T(1)) != 0) {  // (in regime: one ballot)
          mul = 2;
          while (mul < 16 && __ballot(need > T(mul))) ++mul;
        }
        const int nsub = ka.substeps * mul;
        integrate_delta(w.x, w.v, w.q, w.W, dyn, nsub, T(c.dt) * recip(T(nsub)));
      } else if (__ballot(need > T(1)) == 0) {  // in regime: exactly the plain kernel's code path (one ballot)
        const int nsub = ka.substeps;
        integrate_sel<MAG>(w.x, w.v, w.q, w.W, dyn, nsub, T(c.dt) * recip(T(nsub)));
      } else {
        int mul = 2;
        while (mul < 16 && __ballot(need > T(mul))) ++mul;
        const int nsub = ka.substeps * mul;
        integrate_sel<MAG>(w.x, w.v, w.q, w.W, dyn, nsub, T(c.dt) * recip(T(nsub)));
      }
    } else {
      const int nsub = ka.substeps;
      // (one-step helper launch with two or more substeps: priority for the chain from here to the pool barrier, on any grid —
      //  Quad-v0 131 072 envs x 10 substeps 9.66 -> 9.21 us, x 4: 7.04 -> 6.67, x 2: 5.97 -> 5.78; with ONE substep it loses
      //  at 65 536 envs (+1.2 %) and is left out: profiles/r05/ab_step_prio.txt)
      if constexpr (HELP && SINGLE) {
        if (nsub >= kPrioSubsteps) __builtin_amdgcn_s_setprio(kStepPrio);
      }
      integrate_sel<MAG>(w.x, w.v, w.q, w.W, dyn, nsub, kHeadOrder ? hstep : T(c.dt) * recip(T(nsub)));
    }
    renorm_quat(w.q);  //@sec renorm-late-loads-pack
    if constexpr (kLateLoads) {
      const SoA<float> integ(a.integ, 8, L);
#pragma unroll
      for (int f = 0; f < 8; ++f) w.integ[f] = integ.load(f, ufirst, ll);
      if (goal_ptr) {
        const SoA<float> goal(goal_ptr, 12, L);
#pragma unroll
        for (int f = 0; f < 12; ++f) w.goal[f] = goal.load(f, ufirst, ll);
      }
    }
    // The attitude as it is stored (qr_traj.h: QuatPack) is formed once per env-step: here when this wave may store
    // its settled lanes early (below), otherwise after the reset block, when every lane holds what it will store.
    if (early_store) pack_quat(w.q, qp);

    // ---- obs / reward / done ----  //@sec obs-reward-done
    T R[9];
    float o0[D0];
    float o1[D1];
    float rraw[NAG], rwd[NAG];
    bool dn[NAG];
    if constexpr (KIND == QR_KIND_QUAD) {
      if constexpr (kHelpReward) {
        // the helper wave forms and stores the reward (below, after the barrier): hand it the post-step state
        auto& ps = post_lds[SINGLE ? 0 : (t & 1)];
#pragma unroll
        for (int j = 0; j < 3; ++j) { ps.x[j][lane] = w.x[j]; ps.v[j][lane] = w.v[j]; ps.W[j][lane] = w.W[j]; }
#pragma unroll
        for (int j = 0; j < 4; ++j) ps.q[j][lane] = w.q[j];
        dn[0] = quad_done<T, X>(w.x, w.v, w.q, w.W, c);  // (formed while the LDS writes land)
        if constexpr (!SINGLE) ps.done[lane] = dn[0] ? 1u : 0u;
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if constexpr (SINGLE) __builtin_amdgcn_s_setprio(0);
        rraw[0] = rwd[0] = 0.0f;
      } else {
        const float r = quad_reward_raw<T, X>(w.x, w.v, w.q, w.W, w.goal, c);
        rraw[0] = r;
        rwd[0] = interp01(r, c.rmin_mono, c.inv_nrmin_mono);
        dn[0] = quad_done<T, X>(w.x, w.v, w.q, w.W, c);
      }
    } else {
      quat_to_R(w.q, R);
      error_obs<KIND, T, X>(w, R, c, o0, o1);
      // (wrapper_reward_done's formulas, written out: the call reorders four moves in the Coupled helper-wave rollouts — docs/EXPERIMENTS.md "refactor")
      if constexpr (KIND == QR_KIND_COUPLED) {  // coupled:78-110, float32 arithmetic on the float32 obs
        const float r = -c.Cx * sq3(&o0[0]) + -c.CIx * sq3(&o0[3]) + -c.Cv * sq3(&o0[6]) +
                        -c.Cb1 * fabsf(o0[18]) + -c.CIb1 * (o0[19] * o0[19]) + -c.CW * sq3(&o0[20]);
        rraw[0] = r;
        rwd[0] = interp01(r, c.rmin_mono, c.inv_nrmin_mono);
        dn[0] = out3(&o0[0]) | out3(&o0[6]) | out3(&o0[20]);
      } else {  // decoupled:92-140
        const float r1 = -c.Cx * sq3(&o0[0]) + -c.CIx * sq3(&o0[3]) + -c.Cv * sq3(&o0[6]) + -c.Cw12 * sq3(&o0[12]);
        const float r2 = -c.Cb1 * fabsf(o1[0]) + -c.CIb1 * (o1[1] * o1[1]) + -c.CW3 * (o1[2] * o1[2]);
        rraw[0] = r1; rraw[NAG - 1] = r2;
        rwd[0] = interp01(r1, c.rmin_1, c.inv_nrmin_1); rwd[NAG - 1] = interp01(r2, c.rmin_2, c.inv_nrmin_2);
        dn[0] = out3(&o0[0]) | out3(&o0[6]) | out3(&o0[12]);
        dn[NAG - 1] = !(fabsf(o1[2]) < 1.0f);
      }
    }
    if constexpr (kEarlyTile) obs_to_lds<KIND>(o0, o1, smem, smem1, tid);
    // crash override (quad.py:162-166)
#pragma unroll
    for (int g = 0; g < NAG; ++g)
      if (dn[g]) rwd[g] = -1.0f;

    // ---- time limit + auto-reset ----  //@sec reward-done-stores
    steps += 1;
    const bool trunc = ka.max_episode_steps > 0 && steps >= ka.max_episode_steps;
    bool any_done = trunc;
#pragma unroll
    for (int g = 0; g < NAG; ++g) any_done = any_done | dn[g];
    const bool need_reset = auto_reset && any_done && active;
    const int64_t row0 = (int64_t)t * N + first;
    // ---- reward / done of step t (they belong to the step that just ended, whatever the reset does next) ----
    if (active) {
      if constexpr (NAG == 1) {
        if constexpr (!kHelpReward) {
          gstore<AUX>(ka.reward + row0 + lane, rwd[0]);
          if (ka.reward_raw) gstore<AUX>(ka.reward_raw + row0 + lane, rraw[0]);
        }
        gstore<AUX>(done_ptr + row0 + lane, (uint8_t)(dn[0] ? 1 : 0));
      } else {
        gstore<AUX>(reinterpret_cast<float2*>(ka.reward) + row0 + lane, make_float2(rwd[0], rwd[NAG - 1]));
        if (ka.reward_raw) gstore<AUX>(reinterpret_cast<float2*>(ka.reward_raw) + row0 + lane, make_float2(rraw[0], rraw[NAG - 1]));
        gstore<AUX>(reinterpret_cast<uchar2*>(done_ptr) + row0 + lane, make_uchar2(dn[0] ? 1 : 0, dn[NAG - 1] ? 1 : 0));
      }
      if (trunc_ptr) gstore<AUX>(trunc_ptr + row0 + lane, (uint8_t)(trunc ? 1 : 0));
    }
    // (HELP) the helper wave's pool is in LDS: it got there while this wave waited for its loads.  A bare s_barrier:
    // nothing of this wave's own (its reward / done stores in flight) has to be waited for.
    if constexpr (kRollRows) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // (+ the previous step's tile has landed)
    else if constexpr (HELP && !kHelpReward) asm volatile("s_barrier" ::: "memory");
    if constexpr (HELP && !kHelpReward && SINGLE) __builtin_amdgcn_s_setprio(0);
    const unsigned long long rmask = __ballot(need_reset);
    if (rmask) {  // wave-uniform: skipped unless some lane of this wave starts a new episode  //@sec reset-block
      if (early_store) {
        // This wave is about to spend ~0.5 us sampling episode starts.  The state of its lanes that do NOT
        // reset is final: hand it to the memory system first, so that those stores drain meanwhile.  Only for
        // grids in the launch-latency regime: the resetting lanes' own stores then are partial-line writes, which
        // cost more than the overlap gains once the launch is bound by bytes (measured, bench.py: 65 536 envs 5.43
        // with / 5.49 us without; 1 M envs 39.4 with / 37.4 us without).
        if (active && !need_reset) {
          store_state<XV, QW, AUX>(a, first, lane, w, qp);
          if (KIND != QR_KIND_QUAD) {
            const SoA<float> integ(a.integ, 8, L);
#pragma unroll
            for (int f = 0; f < 8; ++f) integ.store<AUX>(f, ufirst, lane, w.integ[f]);
          }
        }
        stored_early = active && !need_reset;
      }
      // the terminal observation of the episode that ends here (what a learner bootstraps from):
      // written for the resetting lanes only
      if (need_reset && ka.final_obs0 != nullptr) {
        if constexpr (KIND == QR_KIND_QUAD) {
          T Rf[9];
          quat_to_R(w.q, Rf);
          float* fo = ka.final_obs0 + (row0 + lane) * D0;
#pragma unroll
          for (int j = 0; j < 3; ++j) { gstore<AUX>(fo + j, (float)w.x[j]); gstore<AUX>(fo + 3 + j, (float)w.v[j]); gstore<AUX>(fo + 15 + j, (float)w.W[j]); }
#pragma unroll
          for (int j = 0; j < 9; ++j) gstore<AUX>(fo + 6 + j, (float)Rf[j]);
        } else {
          float* fo = ka.final_obs0 + (row0 + lane) * D0;
#pragma unroll
          for (int j = 0; j < D0; ++j) gstore<AUX>(fo + j, kEarlyTile ? smem[tid * D0 + j] : o0[j]);
          if constexpr (KT::D1 > 0) {
            float* f1 = ka.final_obs1 + (row0 + lane) * D1;
#pragma unroll
            for (int j = 0; j < D1; ++j) gstore<AUX>(f1 + j, kEarlyTile ? smem1[tid * D1 + j] : o1[j]);
          }
        }
      }
      const int rank = __popcll(rmask & ((1ull << lane) - 1ull));  // rank among the wave's resetting lanes
      const int total = __popcll(rmask);
      uint32_t r19 = 0;
      int pass0 = 0;
      if constexpr (HELP) {  // pass 0 comes from the helper wave
        take_from_lds<T, X, TRAJ != 0>(pool_lds[(SINGLE || POLICY) ? 0 : (t & 1)], need_reset && rank < 12, rank, w, r19);
        pass0 = 1;
        if (total > 12) {  // more than 12 lanes reset at once (rare): this wave samples the further passes itself
          pool_role(role, randomise, eval_reset, c);
          rcount_s = (uint32_t)reset_count[tile_id];  // (still this launch's base: advanced only at the end)
        }
      }
      // (one-step launches) the lane's role constants are formed HERE, not while the loads are in flight: twelve values
      // held across the whole step cost the plain kernel its fourth wave per SIMD (142 -> 128 VGPRs), and the grids that
      // run it are either large (other waves cover this) or take the helper-wave instantiation.
      if (kLazyRole && !HELP) pool_role(role, randomise, eval_reset, c);
      for (int pass = pass0; 12 * pass < total; ++pass) {  // one pass unless more than 12 lanes reset at once
        const int slot = rank - 12 * pass;
#if defined(__HIP_DEVICE_COMPILE__)
        // (multi-step kernels) keep the Philox key schedule — 20 seed-derived words — out of the step loop's preamble: made opaque
        // HERE, the seed's derived values are formed where this rare path uses them instead of being hoisted out of the loop and
        // spilled into VGPR lanes that the loop then reads back (in-loop v_readlane: Quad-v0 rollout 26 -> 13, Coupled actor rollout
        // 14 -> 3; bit-identical, rollouts 1-2 % faster: profiles/r05/ab_local_keys.txt)
        uint64_t seed_here = seed, gfirst_here = gfirst;
        if constexpr (!SINGLE) asm volatile("" : "+s"(seed_here), "+s"(gfirst_here));
        make_pool<T>(pool, role, seed_here, gfirst_here, rcount_s + (uint32_t)t, pass);
#else
        make_pool<T>(pool, role, seed, gfirst, rcount_s + (uint32_t)t, pass);
#endif
        // through LDS (six 16-byte reads per taking lane) rather than 23 ds_bpermute with all their results in flight at
        // once: 128 instead of 142 VGPRs for the plain Quad-v0 kernel, i.e. four waves per SIMD instead of three
        pool_to_lds(own_pool, pool);
        tile_sync<B>();
        take_from_lds<T, X, TRAJ != 0>(own_pool, need_reset && slot >= 0 && slot < 12, slot, w, r19);
        tile_sync<B>();
      }
      if (need_reset) {
        // (with a params buffer the float32 words about to be stored are also what the following steps of a rollout use,
        // randomised or not: exactly what a one-step launch re-loads)
        w.nominal = a.params == nullptr;
        if (a.params != nullptr) params_dirty = true;
        // episode counter (stream id of qr_reset / qr_traj_start): fire-and-forget, nothing here waits for it
        __hip_atomic_fetch_add(ka.episode + i, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        steps = 0;
        if constexpr (TRAJ) {  // mark_traj_start + first get_desired of the episode (main.py:227-229)
          float th, tt, wb, b1d_dot[3];
          traj_draws(r19, th, tt, wb);
          traj_start<kStateful>(w, tr, goal_mode, th, tt, wb);
          traj_goal<kStateful>(w, tr, goal_mode, c, b1d_dot);
          traj_dirty = true;
        }
        if constexpr (KIND != QR_KIND_QUAD) {
          quat_to_R(w.q, R);
#pragma unroll
          for (int f = 0; f < 8; ++f) w.integ[f] = 0.0f;
          error_obs<KIND, T, X>(w, R, c, o0, o1);  // first observation of the new episode (main.py:226-230)
          if constexpr (kEarlyTile) obs_to_lds<KIND>(o0, o1, smem, smem1, tid);
        }
        if (early_store) pack_quat(w.q, qp);
      }
      if constexpr (kHoistAct) act_consts(w, c, ac);  // (some lane of the wave holds new parameters: every lane re-forms — the same values for the others)
    }
    if (!early_store) pack_quat(w.q, qp);  //@sec pack-quat

    // ---- outputs of step t ----  //@sec obs-rows-out
    if constexpr (kHelpRows) {  // rows -> LDS tile(s); the helper wave stores them
      if (KIND != QR_KIND_QUAD || ka.obs0 != nullptr) {
        if constexpr (KIND == QR_KIND_QUAD) {  // next state in the reference's order (x, v, vec_F(R), W)
          quat_to_R(w.q, R);
          quad_state_row(w.x, w.v, R, w.W, o0);
        }
        if constexpr (!kEarlyTile) obs_to_lds<KIND>(o0, o1, smem, smem1, tid);
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      }
    } else if constexpr (kEarlyTile) {  // (plain one-step wrapper kernel) the tile(s) are complete: carry them out
      tile_sync<B>();
      lds_to_rows<B, D0, AUX>(ka.obs0 + row0 * D0, smem, tid, rows);
      if constexpr (KT::D1 > 0) lds_to_rows<B, D1, AUX>(ka.obs1 + row0 * D1, smem1, tid, rows);
    } else if constexpr (HELP && POLICY != 0) {  // the tile is next step's MFMA operand AND this step's rows (helper wave)
      obs_to_lds<KIND>(o0, o1, smem, smem1, tid);
      tile_sync<B>();
    } else if constexpr (kRollRows) {  // tile t & 1; the helper carries it out behind the next pool barrier
      obs_to_lds<KIND>(o0, o1, rtile0 + (t & 1) * (B * D0), rtile1 + (t & 1) * (B * D1), tid);
    } else {
    if constexpr (KIND == QR_KIND_QUAD) {
      if (ka.obs0 != nullptr) {  // next state in the reference's order (x, v, vec_F(R), W)
        quat_to_R(w.q, R);
        quad_state_row(w.x, w.v, R, w.W, o0);
        store_rows<B, D0, AUX>(ka.obs0 + row0 * D0, o0, smem, tid, rows);
      }
    } else {
      store_rows<B, D0, AUX>(ka.obs0 + row0 * D0, o0, smem, tid, rows);
    }
    if constexpr (KT::D1 > 0) store_rows<B, D1, AUX>(ka.obs1 + row0 * D1, o1, smem, tid, rows);
    }
    if constexpr (POLICY) {
#pragma unroll
      for (int j = 0; j < D0; ++j) po0[j] = o0[j];
#pragma unroll
      for (int j = 0; j < D1; ++j) po1[j] = o1[j];
    }
    if constexpr (!SINGLE) unpack_quat(qp, w.q);  //@sec unpack-quat  // the next env-step starts from what a single-step launch would have re-loaded
  }

  if constexpr ((HELP && POLICY != 0) || kRollRows) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // the last step's tile: see the helper wave
  // ---- write the working set back ----  //@sec epilogue-stores
  if (active) {
    if (!(SINGLE && stored_early)) {
      store_state<XV, QW, AUX>(a, first, lane, w, qp);
      if (KIND != QR_KIND_QUAD) {
        const SoA<float> integ(a.integ, 8, L);
#pragma unroll
        for (int f = 0; f < 8; ++f) integ.store<AUX>(f, ufirst, lane, w.integ[f]);
      }
    }
    if (steps_ptr) gstore<AUX>(steps_ptr + first + lane, steps);
    if constexpr (TRAJ) {
      const SoA<float> traj(ka.traj, 8, L);
      traj.store<AUX>(0, ufirst, lane, tr.calls);
      if (traj_dirty || kStateful) {  // the rest changes only at a reset — or, in the stateful modes, with any call
#pragma unroll
        for (int f = 1; f < (kStateful ? 8 : 7); ++f) traj.store<AUX>(f, ufirst, lane, tr.get(f));
      }
      if constexpr (kStateful) {
        const SoA<float> goal(goal_ptr, 12, L);
#pragma unroll
        for (int f = 0; f < 12; ++f) goal.store<AUX>(f, ufirst, lane, w.goal[f]);
      }
    }
    if (params_dirty) {
      const SoA<float> prm(a.params, 6, L);
#pragma unroll
      for (int f = 0; f < 6; ++f) prm.store<AUX>(f, ufirst, lane, w.prm[f]);
    }
  }
  if constexpr (HELP) {  // (the helper wave read the counter; this wave only advances it)
    if (lane == 0) __hip_atomic_fetch_add(a.reset_count + tile_id, n_steps, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else if (auto_reset && lane == 0) {
    a.reset_count[tile_id] = (int32_t)(rcount_s + (uint32_t)n_steps);  // never reuse a (tile, counter)
  }
  QR_SPAN_END();
}

}  // namespace qr
