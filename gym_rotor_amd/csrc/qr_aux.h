// qr_aux.h — part of the gfx950 quadrotor step library (included by quadrotor_kernels.hip, in this order).
// Auxiliary kernels: error observation, reset, state get / set, goal generator start / query, qr_touch, GAE.
#pragma once
#include "qr_step.h"

namespace qr {

// get_norm_error_state on the current state (quad.py:421-466)
template <int KIND, typename XV, typename QW>
__global__ __launch_bounds__(64) void error_obs_kernel(const Args a) {
  using T = QW;
  using KT = KindTraits<KIND>;
  constexpr int B = 64, D0 = KT::D0, D1 = KT::D1 ? KT::D1 : 1;
  __shared__ __attribute__((aligned(16))) float smem[B * D0];
  const int tid = threadIdx.x;
  const int64_t first = (int64_t)blockIdx.x * B;
  const int64_t i = first + tid;
  const int64_t N = a.n, L = a.ld;
  const int rows = (int)((N - first) < B ? (N - first) : B);
  const bool active = tid < rows;
  Work<T, XV> w;
  idle_work(w, a.c);
  if (active) {
    load_state<XV, QW>(a, first, (unsigned)tid, w);
    if (a.goal) {
#pragma unroll
      for (int f = 0; f < 12; ++f) w.goal[f] = a.goal[(int64_t)f * L + i];
    }
#pragma unroll
    for (int f = 0; f < 8; ++f) w.integ[f] = a.integ[(int64_t)f * L + i];
  }
  T R[9];
  quat_to_R(w.q, R);
  float o0[D0];
  float o1[D1];
  error_obs<KIND, T, XV>(w, R, a.c, o0, o1);
  store_rows<B, D0>(a.obs0 + first * D0, o0, smem, tid, rows);
  if constexpr (KT::D1 > 0) store_rows<B, D1>(a.obs1 + first * D1, o1, smem, tid, rows);
  if (active) {
#pragma unroll
    for (int f = 0; f < 8; ++f) a.integ[(int64_t)f * L + i] = w.integ[f];
  }
}

// QuadEnv.reset for masked envs
template <typename XV, typename QW>
__global__ __launch_bounds__(64) void reset_kernel(const Args a) {
  using T = QW;
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const int64_t N = a.n, L = a.ld;
  if (i >= N) return;
  if (a.mask && !a.mask[i]) return;
  const int32_t episode = a.episode[i] + 1;
  const bool eval = (a.flags & QR_FLAG_EVAL_RESET) != 0;
  const bool randomise = !eval && !(a.flags & QR_FLAG_NO_UDM);
  Work<T, XV> w;
  Draws d;
  draw20(d, a.seed, (uint64_t)(a.env_offset + i), (uint32_t)episode);
  sample_reset(w, d, randomise, eval, a.c);
  store_state<XV, QW>(a, (int64_t)blockIdx.x * 64, threadIdx.x, w);
  if (a.params) {
#pragma unroll
    for (int f = 0; f < 6; ++f) a.params[(int64_t)f * L + i] = w.prm[f];
  }
  if (a.integ) {
#pragma unroll
    for (int f = 0; f < 8; ++f) a.integ[(int64_t)f * L + i] = 0.f;
  }
  if (a.steps) a.steps[i] = 0;
  a.episode[i] = episode;
}

// get_current_state: 13-word internal state -> the reference's float64 18-vector rows
template <typename XV, typename QW>
__global__ __launch_bounds__(64) void get_state_kernel(const Args a) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= a.n) return;
  Work<QW, XV> w;
  load_state<XV, QW>(a, (int64_t)blockIdx.x * 64, threadIdx.x, w);
  double q[4], R[9];
#pragma unroll
  for (int j = 0; j < 4; ++j) q[j] = (double)w.q[j];
  quat_to_R(q, R);
  quad_state_row(w.x, w.v, R, w.W, *reinterpret_cast<double (*)[18]>(a.rows_out + i * 18));
}

// state injection: float64 18-vector rows -> 13-word internal state (R -> nearest rotation -> q).
// A row whose attitude block has no nearest rotation in SO(3) (det R <= 0, or non-finite entries:
// quad_utils.py:123-142 would hand such an R to the SVD and return a reflection-corrected matrix
// that has nothing to do with the input) is REJECTED: the env keeps its state and the row is
// counted in *status, which the host side turns into an error.
template <typename XV, typename QW>
__global__ __launch_bounds__(64) void set_state_kernel(const Args a) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= a.n) return;
  if (a.mask && !a.mask[i]) return;
  const double* r = a.rows_in + i * 18;
  Work<QW, XV> w;
#pragma unroll
  for (int j = 0; j < 3; ++j) { w.x[j] = (XV)r[j]; w.v[j] = (XV)r[3 + j]; w.W[j] = (QW)r[15 + j]; }
  double q[4];
  const bool ok = R_to_quat(r + 6, q);
  if (!ok) {
    if (a.status) atomicAdd(a.status, 1);
    return;
  }
  if (a.dry_run) return;  // (qr_check_state: the same decision, nothing written)
#pragma unroll
  for (int j = 0; j < 4; ++j) w.q[j] = (QW)q[j];
  store_state<XV, QW>(a, (int64_t)blockIdx.x * 64, threadIdx.x, w);
}

// mark_traj_start for masked envs, from the current state
template <typename XV, typename QW>
__global__ __launch_bounds__(64) void traj_start_kernel(const Args a) {
  using T = QW;
  const int64_t first = (int64_t)blockIdx.x * 64;
  const unsigned lane = threadIdx.x;
  const int64_t i = first + lane;
  if (i >= a.n) return;
  if (a.mask && !a.mask[i]) return;
  Work<T, XV> w;
  load_state<XV, QW>(a, first, lane, w);
  float th, tt, wb;
  if (a.draws) {
    th = a.draws[i]; tt = a.draws[a.n + i]; wb = a.draws[2 * a.n + i];
  } else {
    Draws d;
    draw20(d, a.seed, (uint64_t)(a.env_offset + i), (uint32_t)a.episode[i]);
    traj_draws(d.r[19], th, tt, wb);
  }
  Traj tr;
  if (a.goal_mode >= QR_GOAL_MODE2) traj_start<true>(w, tr, a.goal_mode, th, tt, wb);
  else traj_start<false>(w, tr, a.goal_mode, th, tt, wb);
  const SoA<float> traj(a.traj, 8, a.ld);
#pragma unroll
  for (int f = 0; f < 8; ++f) traj.store(f, (unsigned)first, lane, tr.get(f));
  if (a.goal_mode >= QR_GOAL_MODE2) {  // the stateful modes: the persistent fields of a fresh generator
    const SoA<float> goal(a.goal, 12, a.ld);
#pragma unroll
    for (int f = 0; f < 12; ++f) goal.store(f, (unsigned)first, lane, w.goal[f]);
  }
}

// get_desired for the current state: rows [N][15] = xd, vd, b1d, b1d_dot, Wd
template <typename XV, typename QW>
__global__ __launch_bounds__(64) void get_desired_kernel(const Args a) {
  using T = QW;
  const int64_t first = (int64_t)blockIdx.x * 64;
  const unsigned lane = threadIdx.x;
  const int64_t i = first + lane;
  if (i >= a.n) return;
  if (a.mask && !a.mask[i]) return;
  Work<T, XV> w;
  idle_work(w, a.c);
  load_state<XV, QW>(a, first, lane, w);
  const SoA<float> traj(a.traj, 8, a.ld);
  Traj tr;
#pragma unroll
  for (int f = 0; f < 8; ++f) tr.set(f, traj.load(f, (unsigned)first, lane));
  const bool stateful = a.goal_mode >= QR_GOAL_MODE2;  // modes 2-5: xd, vd, b1d, Wd persist in the goal buffer
  if (stateful) {
    const SoA<float> goal(a.goal, 12, a.ld);
#pragma unroll
    for (int f = 0; f < 12; ++f) w.goal[f] = goal.load(f, (unsigned)first, lane);
  }
  float b1d_dot[3];
  if (stateful) traj_goal<true>(w, tr, a.goal_mode, a.c, b1d_dot);
  else traj_goal<false>(w, tr, a.goal_mode, a.c, b1d_dot);
  traj.store(0, (unsigned)first, lane, tr.calls);
  if (stateful) {
#pragma unroll
    for (int f = 1; f < 8; ++f) traj.store(f, (unsigned)first, lane, tr.get(f));
  }
  if (a.goal_rows) {
    float* o = a.goal_rows + i * 15;
#pragma unroll
    for (int j = 0; j < 9; ++j) o[j] = w.goal[j];
#pragma unroll
    for (int j = 0; j < 3; ++j) { o[9 + j] = b1d_dot[j]; o[12 + j] = w.goal[9 + j]; }
  }
  if ((a.store_goal || stateful) && a.goal) {
    const SoA<float> goal(a.goal, 12, a.ld);
#pragma unroll
    for (int f = 0; f < 12; ++f) goal.store(f, (unsigned)first, lane, w.goal[f]);
  }
}

// ------------------------------------------------------------------------------------
// qr_touch: the step's memory traffic and nothing else — the yardstick bench.py prices a step against (roofline.noop_kernel_us).
// Per env exactly what qr_step moves: state in and out (same SoA accesses, same widths), parameters, action row, [goal],
// [integrator words in and out], [observation rows out], reward and done rows out; no arithmetic beyond one sum that keeps
// the loads alive.  One wavefront per 64-env tile, plain stores.  The state is written back as read (bit for bit); the
// output rows hold zeros afterwards.
// ------------------------------------------------------------------------------------
template <int KIND, typename XV, typename QW>
__global__ __launch_bounds__(64) void touch_kernel(void* pos_vel, void* att_rate, const float* action, float* params, float* integ_ptr, float* reward,
                                                   int32_t n_envs, int32_t ld_envs, const Args a_in) {
  // (like step_kernel: what the first loads need arrives in preloaded SGPRs, the rest is read from the kernarg segment where it is used)
#if defined(__HIP_DEVICE_COMPILE__)
  const Args& a = *reinterpret_cast<const Args*>(reinterpret_cast<const char*>(__builtin_amdgcn_kernarg_segment_ptr()) + kArgsOffset);
  (void)a_in;
#else
  const Args& a = a_in;
#endif
  using KT = KindTraits<KIND>;
  constexpr int A = KT::A, D0 = KT::D0, D1 = KT::D1, NAG = KT::NAG;
  // the output pointers, read with the wave's first scalar loads (not at the very end, where a scalar-cache miss on the kernarg
  // segment would hold the wave's registers: the plain step kernel does the same, qr_step.h "done_ptr")
  uint8_t* const done_ptr = a.done;
  float* const obs0_ptr = a.obs0;
  float* const obs1_ptr = KT::D1 > 0 ? a.obs1 : nullptr;
  float* const goal_ptr = KIND != QR_KIND_QUAD ? a.goal : nullptr;
  const unsigned first = blockIdx.x * 64u, lane = threadIdx.x;
  const int rows = min(n_envs - (int)first, 64);
  const unsigned ll = min(lane, (unsigned)(rows - 1));
  const bool active = (int)lane < rows;
  const SoA<XV> pv(pos_vel, 6, ld_envs);
  const SoA<QW> ar(att_rate, 6, ld_envs);
  const SoA<float> prm(params, 6, ld_envs), integ(integ_ptr, 8, ld_envs), goal(goal_ptr, 12, ld_envs);
  XV x[6]; QW q[6]; float ig[8], pr[6], ac[A], gl[12];
  float s = 0.0f;
  // every load of the wave is issued before anything waits (one batch, like the step kernel's prologue)
#pragma unroll
  for (int f = 0; f < 6; ++f) q[f] = ar.load(f, first, ll);
#pragma unroll
  for (int f = 0; f < 6; ++f) x[f] = pv.load(f, first, ll);
#pragma unroll
  for (int f = 0; f < 6; ++f) pr[f] = prm.load(f, first, ll);
  load_action_row(action + (int64_t)first * A, ll, ac);
  const bool has_goal = KIND != QR_KIND_QUAD && goal_ptr != nullptr;
  if constexpr (KIND != QR_KIND_QUAD) {
#pragma unroll
    for (int f = 0; f < 8; ++f) ig[f] = integ.load(f, first, ll);
    if (has_goal) {
#pragma unroll
      for (int f = 0; f < 12; ++f) gl[f] = goal.load(f, first, ll);
    } else {
#pragma unroll
      for (int f = 0; f < 12; ++f) gl[f] = 0.0f;
    }
  }
  asm volatile("" ::"s"(done_ptr), "s"(obs0_ptr), "s"(obs1_ptr));   // (the scalar batch is waited for HERE: behind the vector loads' issue)
  // (pinned: left alone, the compiler sinks the state loads into the `active` block below, BEHIND the wait for the parameter and
  // action loads — two dependent round trips per wave instead of one batch: 28.7 instead of 24.7 us at 1 M envs)
#pragma unroll
  for (int f = 0; f < 6; ++f) asm volatile("" : "+v"(q[f]), "+v"(x[f]), "+v"(pr[f]));
#pragma unroll
  for (int j = 0; j < A; ++j) asm volatile("" : "+v"(ac[j]));
  if constexpr (KIND != QR_KIND_QUAD) {
#pragma unroll
    for (int f = 0; f < 8; ++f) asm volatile("" : "+v"(ig[f]));
#pragma unroll
    for (int f = 0; f < 12; ++f) { asm volatile("" : "+v"(gl[f])); s += gl[f]; }
  }
#pragma unroll
  for (int f = 0; f < 6; ++f) s += pr[f];
#pragma unroll
  for (int j = 0; j < A; ++j) s += ac[j];
  s = s * 0.0f;  // (0 for finite inputs; not foldable without fast-math, so the loads stay)
  if (active) {
#pragma unroll
    for (int f = 0; f < 6; ++f) ar.store(f, first, lane, q[f]);
#pragma unroll
    for (int f = 0; f < 6; ++f) pv.store(f, first, lane, x[f]);
    if constexpr (KIND != QR_KIND_QUAD) {
#pragma unroll
      for (int f = 0; f < 8; ++f) integ.store(f, first, lane, ig[f]);
    }
    if constexpr (NAG == 1) reward[first + lane] = s;
    else reinterpret_cast<float2*>(reward)[first + lane] = make_float2(s, s);
    if constexpr (NAG == 1) done_ptr[first + lane] = 0;
    else reinterpret_cast<uchar2*>(done_ptr)[first + lane] = make_uchar2(0, 0);
  }
  auto rows_out = [&](float* base, int D) {  // the tile's rows as they lie in memory: 16-byte stores, like lds_to_rows
    if (base == nullptr) return;
    float* g = base + (int64_t)first * D;
    if (rows == 64 && (reinterpret_cast<uintptr_t>(g) & 15u) == 0) {
      for (int idx = (int)lane; idx < 16 * D; idx += 64) reinterpret_cast<float4*>(g)[idx] = make_float4(s, s, s, s);
    } else {
      for (int idx = (int)lane; idx < rows * D; idx += 64) g[idx] = s;
    }
  };
  rows_out(obs0_ptr, D0);
  if constexpr (D1 > 0) rows_out(obs1_ptr, D1);
}

// ------------------------------------------------------------------------------------
// GAE reverse scan (algos/ppo/ppo.py:134-146): one lane per (env, agent) column, T steps.
// The recurrence is serial in t but the loads are not: they are issued kU steps ahead so that
// a wave keeps kU rows in flight instead of paying one memory round-trip per step.
// ------------------------------------------------------------------------------------
struct GaeArgs {
  const float* reward; const uint8_t* done; const float* value; const float* next_value;
  float* advantage; float* td_target; double* partials;
  int64_t m; int32_t T; float gamma; float lam;
};

__global__ __launch_bounds__(64) void gae_kernel(const GaeArgs g) {
  constexpr int kU = 8;
  const int64_t j = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const bool active = j < g.m;
  const int64_t M = g.m;
  float adv = 0.0f;
  double s1 = 0.0, s2 = 0.0;
  if (active) {
    float vnext = g.next_value ? 0.0f : g.value[(int64_t)g.T * M + j];  // bootstrap row
    for (int t0 = g.T; t0 > 0; t0 -= kU) {
      const int nb = t0 < kU ? t0 : kU;
      float r[kU], v[kU], vn[kU];
      uint8_t d[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        if (u < nb) {
          const int64_t idx = (int64_t)(t0 - 1 - u) * M + j;
          r[u] = g.reward[idx]; d[u] = g.done[idx]; v[u] = g.value[idx];
          vn[u] = g.next_value ? g.next_value[idx] : 0.0f;
        }
      }
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        if (u < nb) {
          const int64_t idx = (int64_t)(t0 - 1 - u) * M + j;
          const float nd = d[u] ? 0.0f : 1.0f;
          const float vnx = g.next_value ? vn[u] : vnext;
          const float delta = r[u] + g.gamma * vnx * nd - v[u];
          adv = delta + g.gamma * nd * g.lam * adv;
          g.advantage[idx] = adv;
          g.td_target[idx] = adv + v[u];
          s1 += (double)adv; s2 += (double)adv * (double)adv;
          vnext = v[u];
        }
      }
    }
  }
  if (g.partials) {  // wave reduction (DPP/bpermute shuffles), one pair of doubles per workgroup
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { s1 += __shfl_down(s1, off); s2 += __shfl_down(s2, off); }
    if (threadIdx.x == 0) { g.partials[2 * (int64_t)blockIdx.x] = s1; g.partials[2 * (int64_t)blockIdx.x + 1] = s2; }
  }
}

}  // namespace qr
