// qr_sac.h — part of the gfx950 quadrotor step library (included by quadrotor_kernels.hip only, after qr_td3_actor.h).
// The piece of SAC's critic update (SAC.train, algos/sac/sac.py:135-153, the non-CTDE branch) that the TD3 kernels cannot form: the
// soft target values of a minibatch in ONE launch, with j the minibatch position and i = index[j]:
//   sac_target_kernel  (qr_sac_target)   mean, ls = pi(obs_next[i]);  ls = clamp(ls, -20, 2)            (the LIVE actor)
//                                        u = mean + exp(ls) eps[j];   a' = tanh(u)
//                                        logp_j = sum_f [ -eps^2/2 - ls - log sqrt(2 pi) - log(1 - a'^2 + 1e-6) ]
//                                        y[j] = reward[i] + discount (1 - done[i]) (min(Q1_targ, Q2_targ)(obs_next[i], a') - alpha logp_j)
// The regression against y and its twelve gradients are qr_twinq_grad's (qr_td3.h), the Polyak step qr_soft_update's.
// The tile walk — staging, the actor's heads, both target networks — is target_walk's (qr_td3.h), shared with td3_target_kernel; here:
// the sample (sac_sample) and SacRule, what the walk asks of SAC.
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

// Per-agent members are arrays of two, as Td3TargetArgs's (qr_td3.h): the one-agent entry fills [0]; the centralized (CTDE) entry
// fills both.  There logp is agent `own`'s alone, from a draw of its own where eps_logp is given (sac.py:139-141 samples that agent twice).
struct SacTargetArgs {
  ActorW actor[2];                   // pi (AD > 0): the LIVE actors, mean head and log_std head; log_std is NULL: never read
  MlpNetW net[2];                    // Q1_targ, Q2_targ
  const float* obs_next[2];          // [>= rows][obs_dim[m]]
  const float *reward, *done;        // element i at [i * rwd_stride] / [i * done_stride]
  const float* eps[2];               // [B][action_dim[m]] by minibatch position, or NULL: zeros
  const float* eps_logp;             // the centralized form: [B][action_dim[own]], or NULL: eps[own]
  const float* action_next[2];       // AD = 0: a' [B][action_dim[m]] by minibatch position, used as it is
  const float* logp_next;            // AD = 0: logp [B] by minibatch position
  const float* alpha_dev;            // device scalar, or NULL: `alpha`
  const int64_t* index;
  float* y;                          // [B]
  float* action_out[2];              // [B][action_dim[m]] or NULL
  float* logp_out;                   // [B] or NULL
  int64_t B, rows;
  int32_t obs_dim[2], action_dim[2], hidden, rwd_stride, done_stride, own;
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

// SAC's rule for target_walk (qr_td3.h): both heads of the LIVE actor, the sample and its log-probability summed over the row, a'
// and logp stored where asked for (supplied ones as copies), the entropy term inside the Bellman line.  Plain stores, no atomics.
struct SacRule {
  using Args = SacTargetArgs;
  static constexpr bool LOG_STD = true;
  const Args& a;
  const float alpha;
  __device__ __forceinline__ explicit SacRule(const Args& args) : a(args), alpha(args.alpha_dev ? args.alpha_dev[0] : args.alpha) {}
  template <bool TWO>
  __device__ __forceinline__ float component(int m, float pre, float ls, int64_t k, bool active, bool own, float& logp) const {
    const float* eps = (TWO && m) ? a.eps[1] : a.eps[0];
    const float z = (eps && active) ? eps[k] : 0.0f;
    float act, lp;
    sac_sample(pre, ls, z, act, lp);
    if constexpr (TWO) {
      if (own && a.eps_logp) {  // the log-probability's own draw: the same function of (pre, ls, e), its action dropped
        float other;
        sac_sample(pre, ls, active ? a.eps_logp[k] : 0.0f, other, lp);
      }
      if (own) logp += lp;
    } else {
      logp += lp;
    }
    return act;
  }
  __device__ __forceinline__ void keep(int m, int64_t k, float act, bool active) const {
    float* out = m ? a.action_out[1] : a.action_out[0];
    if (out && active) out[k] = act;
  }
  __device__ __forceinline__ float supplied(int64_t j, bool active) const { return active ? a.logp_next[j] : 0.0f; }
  __device__ __forceinline__ void bellman(int64_t j, float rwd, float dn, float qmin, float logp) const {
    a.y[j] = fmaf(a.discount * (1.0f - dn), fmaf(-alpha, logp, qmin), rwd);
    if (a.logp_out) a.logp_out[j] = logp;
  }
};

template <int AD, int AD1 = -1>
__global__ __launch_bounds__(64) void sac_target_kernel(const SacTargetArgs a) { target_walk<AD, SacRule, AD1>(a); }

}  // namespace qr
