// qr_sac.h — part of the gfx950 quadrotor step library (included by quadrotor_kernels.hip only, after qr_td3_actor.h).
// The piece of SAC's critic update (SAC.train, algos/sac/sac.py:135-153, the non-CTDE branch) that the TD3 kernels cannot form: the
// soft target values of a minibatch in ONE launch, with j the minibatch position and i = index[j]:
//   sac_target_kernel  (qr_sac_target)   mean, ls = pi(obs_next[i]);  ls = clamp(ls, -20, 2)            (the LIVE actor)
//                                        u = mean + exp(ls) eps[j];   a' = tanh(u)
//                                        logp_j = sum_f [ -eps^2/2 - ls - log sqrt(2 pi) - log(1 - a'^2 + 1e-6) ]
//                                        y[j] = reward[i] + discount (1 - done[i]) (min(Q1_targ, Q2_targ)(obs_next[i], a') - alpha logp_j)
// The regression against y and its twelve gradients are qr_twinq_grad's (qr_td3.h), the Polyak step qr_soft_update's.
// Everything but the sample is reused as it is: stage_rows, twinq_fill_small, load_fc2 and twinq_forward (qr_mlp_grad.h, qr_td3.h),
// both heads of ActorMfma<AD, true> and ActorLds<3, 4, 1> (qr_actor.h).
//
// The tanh correction is NOT formed from the rounded a' (actor_sample's form in the rollout, whose bits are pinned, stays as it is):
// tanh_fast is good to about 2e-7 absolute, which in 1 - a'^2 is a 4e-5 error of the logarithm at |u| = 3 and grows without bound
// beyond.  With t = exp(-2|u|):
//     1 - a'^2 = 4 t / (1 + t)^2          a' = copysign((1 - t) / (1 + t), u)
// the same function with a relative error around 1e-6 at every |u|; the reference's + 1e-6 inside the logarithm stays.  -eps^2/2 is
// formed from eps directly, not as -(u - mean)^2 / (2 var): u - mean cancels as soon as exp(ls) |eps| is small against |mean|.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "quadrotor_hip.h"
#include "qr_actor.h"
#include "qr_td3.h"

namespace qr {

struct SacTargetArgs {
  ActorW actor;                      // pi (AD > 0): the LIVE actor, mean head and log_std head; log_std is NULL: never read
  MlpNetW net[2];                    // Q1_targ, Q2_targ
  const float* obs_next;             // [>= rows][obs_dim]
  const float *reward, *done;        // element i at [i * rwd_stride] / [i * done_stride]
  const float* eps;                  // [B][action_dim] by minibatch position, or NULL: zeros
  const float* action_next;          // AD = 0: a' [B][action_dim] by minibatch position, used as it is
  const float* logp_next;            // AD = 0: logp [B] by minibatch position
  const float* alpha_dev;            // device scalar, or NULL: `alpha`
  const int64_t* index;
  float* y;                          // [B]
  float* action_out;                 // [B][action_dim] or NULL
  float* logp_out;                   // [B] or NULL
  int64_t B, rows;
  int32_t obs_dim, action_dim, hidden, rwd_stride, done_stride;
  float discount, alpha;
};

// One component of MLP_Actor_SAC.sample (sac_mlp.py:65-76) from the heads' outputs: a' and the component's log-probability.
__device__ __forceinline__ void sac_sample(float mean, float log_std, float z, float& act, float& logp) {
  const float ls = fminf(fmaxf(log_std, -20.0f), 2.0f);
  const float u = fmaf(__expf(ls), z, mean);
  const float t = __expf(-2.0f * fabsf(u));
  const float r = __builtin_amdgcn_rcpf(1.0f + t);
  act = copysignf((1.0f - t) * r, u);
  logp = fmaf(-0.5f * z, z, -ls - 0.91893853320467274f) - logf(fmaf(4.0f * t * r, r, 1e-6f));
}

// AD = the actor's obs_dim: 23 or 15 (ActorMfma, hidden 16, 4 actions), 3 (ActorLds<3, 4, 1>), or 0: no actor, a' and logp are
// supplied.  td3_target_kernel's shape: one wavefront per workgroup walks 64-row tiles grid-stride: gather obs_next rows (index,
// clamped) into the critic's input tile and the actor's tile, both heads for the lane's own row, the sample and its log-probability,
// a' into the columns behind the observation, then both target networks over the tile, min, the entropy term and the Bellman line.
// Lane l owns row l.  Plain stores, no atomics.
template <int AD>
__global__ __launch_bounds__(64) void sac_target_kernel(const SacTargetArgs a) {
  constexpr int AA = AD == 3 ? 1 : 4;  // the actor's action_dim
  using Actor1 = ActorLds<3, 4, 1>;
  __shared__ float xs[64 * kMgX];
  __shared__ float as[AD > 0 ? 64 * AD : 4];
  __shared__ __attribute__((aligned(16))) float wsm[AD == 3 ? Actor1::SIZE : 4];
  __shared__ float w1s[2][TwinQL1::SIZE], svec[2][kTqVec];
  __shared__ const float* src0[64];
  const int lane = threadIdx.x;
  const int D = a.obs_dim + a.action_dim, H = a.hidden;
  float q1[4][4][4], q2[4][4][4];  // fc2_w of Q1_targ, Q2_targ
  load_fc2(q1, a.net[0].fc2_w, H, lane);
  load_fc2(q2, a.net[1].fc2_w, H, lane);
  twinq_fill_small(w1s[0], svec[0], a.net[0], D, H, lane);
  twinq_fill_small(w1s[1], svec[1], a.net[1], D, H, lane);
  ActorMfma<(AD == 23 || AD == 15) ? AD : 23, true> actor;
  if constexpr (AD == 23 || AD == 15) actor.load(a.actor, lane);
  if constexpr (AD == 3) Actor1::fill(wsm, a.actor, lane);
  const float alpha = a.alpha_dev ? a.alpha_dev[0] : a.alpha;
  for (int i = lane; i < 64 * kMgX; i += 64) xs[i] = 0.0f;  // the padding columns stay zero: nothing below writes them
  __syncthreads();

  const int64_t tiles = (a.B + 63) / 64;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t row0 = tile * 64, j = row0 + lane;
    const bool active = j < a.B;
    int64_t i = active ? (a.index ? a.index[j] : j) : 0;
    i = i < 0 ? 0 : (i >= a.rows ? a.rows - 1 : i);  // never a read outside the buffer
    src0[lane] = active ? a.obs_next + i * a.obs_dim : nullptr;
    const float rwd = active ? a.reward[i * a.rwd_stride] : 0.0f;
    const float dn = active ? a.done[i * a.done_stride] : 0.0f;
    __syncthreads();
    stage_rows(xs, kMgX, src0, a.obs_dim, 0, lane);
    if constexpr (AD > 0) stage_rows(as, AD, src0, AD, 0, lane);
    __syncthreads();
    float logp = 0.0f;
    if constexpr (AD > 0) {
      float pre[AA], ls[AA];
      if constexpr (AD == 3) {
        float x[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) x[k] = as[lane * 3 + k];
        Actor1::heads(wsm, true, x, pre, ls);
      } else {
        actor.heads(as, lane, pre, ls);
      }
#pragma unroll
      for (int f = 0; f < AA; ++f) {
        const float z = (a.eps && active) ? a.eps[j * AA + f] : 0.0f;
        float act, lp;
        sac_sample(pre[f], ls[f], z, act, lp);
        xs[lane * kMgX + AD + f] = act;
        logp += lp;
        if (a.action_out && active) a.action_out[j * AA + f] = act;
      }
    } else {
      for (int f = 0; f < a.action_dim; ++f) {
        const float act = active ? a.action_next[j * a.action_dim + f] : 0.0f;
        xs[lane * kMgX + a.obs_dim + f] = act;
        if (a.action_out && active) a.action_out[j * a.action_dim + f] = act;  // the outputs, where asked for, are copies
      }
      logp = active ? a.logp_next[j] : 0.0f;
    }
    __syncthreads();
    const float v1 = twinq_forward(q1, xs, lds_here(w1s[0]), lds_here(svec[0]), lane);
    const float v2 = twinq_forward(q2, xs, lds_here(w1s[1]), lds_here(svec[1]), lane);
    __syncthreads();  // the tile is read: the next one may be staged
    if (active) {
      a.y[j] = fmaf(a.discount * (1.0f - dn), fmaf(-alpha, logp, fminf(v1, v2)), rwd);
      if (a.logp_out) a.logp_out[j] = logp;
    }
  }
}

}  // namespace qr
