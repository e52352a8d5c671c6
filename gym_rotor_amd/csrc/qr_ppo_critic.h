// qr_ppo_critic.h — part of the gfx950 quadrotor step library (included by quadrotor_kernels.hip, after qr_ppo.h).
// The critic half of one PPO minibatch update (PPO.train, algos/ppo/ppo.py:193-214): the mean squared error of MLP_Critic /
// MLP_Critic_CTDE against the TD target plus the L2 term on the three weight tensors, and the gradients with respect to the critic's
// six tensors, read from the rollout storage in place: ppo_critic_kernel + ppo_critic_reduce_kernel (qr_ppo_critic_grad).
// The tile walk, the half-tile body, the partial vector and the reduction's sums are qr_mlp_grad.h's, shared with twinq_kernel (qr_td3.h); here,
// as PpoCriticL1 and PcRule: tanh, 24 inputs with fc1_w's operands resident, one or two row sources, the target by storage row, four statistics; the L2 term.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "quadrotor_hip.h"
#include "qr_actor.h"
#include "qr_critic.h"
#include "qr_mlp_grad.h"

namespace qr {

struct PpoCriticArgs {
  MlpNetW w;
  const float *rows0, *rows1;        // [>= rows][in0], [>= rows][in1]: the observation rows (NULL where in0 / in1 is 0)
  const float* target;               // element i at target[i * tgt_stride]
  const int64_t* index;              // [B] or NULL (rows 0..B-1)
  double* partials;                  // [grid][np]
  int64_t B, rows;
  int32_t in0, in1, hidden, tgt_stride;
  float g_scale;                     // 2 / B: dLoss / dv = g_scale * e
};

constexpr int kPcSums = 4;  // the statistics behind the gradients in a partial vector: sum e^2, sum e, sum y, sum y^2

// mlp_grad_half's traits: tanh; 24 inputs (6 k-steps), the ones in column 24; fc1_w resident as A operands.
struct PpoCriticL1 {
  static constexpr int KS = 6, ONES = kCriticIn, XS = kCriticIn;
  float w1[4][KS];

  static __device__ __forceinline__ float act(float z) { return tanh_fast(z); }
  static __device__ __forceinline__ float dact(float t, float d) { return d * fmaf(-t, t, 1.0f); }
  __device__ __forceinline__ float a1(int hb, int s, int) const { return w1[hb][s]; }

  __device__ __forceinline__ void load(const float* fc1_w, int D, int H, int lane) {
    const int c = lane & 15, g = lane >> 4;
#pragma unroll
    for (int hb = 0; hb < 4; ++hb) {
#pragma unroll
      for (int s = 0; s < KS; ++s) w1[hb][s] = (16 * hb + c < H && 4 * s + g < D) ? fc1_w[(16 * hb + c) * D + 4 * s + g] : 0.0f;
    }
  }
};

// mlp_grad_walk's rule (qr_mlp_grad.h): one network, one or two row sources of which an empty one is skipped, fc1_w's operands
// resident in the rule itself (no LDS behind them), the target by storage row, four statistics.
struct PcRule {
  using Args = PpoCriticArgs;
  using L1 = PpoCriticL1;
  static constexpr int SUMS = kPcSums, W1S = 1, SVEC = kMgB3;
  static constexpr int SRC = 2;
  static constexpr bool SKIP_EMPTY = true;
  L1 l1;
  static __device__ __forceinline__ int width(const Args& a, int s) { return s ? a.in1 : a.in0; }
  static __device__ __forceinline__ const MlpNetW& net(const Args& a) { return a.w; }
  __device__ __forceinline__ void fill(float*, float* svec, const MlpNetW& w, int D, int H, int lane) { l1.load(w.fc1_w, D, H, lane); fill_vecs(svec, w, H, lane); }
  __device__ __forceinline__ const L1& layer1(const float*) const { return l1; }
  static __device__ __forceinline__ const float* row(const Args& a, int64_t i, int s) { return s ? a.rows1 + i * a.in1 : a.rows0 + i * a.in0; }
  static __device__ __forceinline__ float target(const Args& a, int64_t i, int64_t) { return a.target[i * a.tgt_stride]; }
  static __device__ __forceinline__ void stat(double (&st)[SUMS], float e, float y) { st[0] += (double)e * (double)e; st[1] += (double)e; st[2] += (double)y; st[3] += (double)y * (double)y; }
};

// (a CTDE row is formed in the walk's tile from its two sources; ppo_critic_reduce_kernel sums the workgroups' partial vectors)
__global__ __launch_bounds__(64) void ppo_critic_kernel(const PpoCriticArgs a) { mlp_grad_walk<PcRule>(a); }

struct PpoCriticReduceArgs {
  const double* partials;   // [n_parts][np]
  const float* weight[3];   // fc1_w, fc2_w, fc3_w: the L2 term
  float* grad[6];           // fc1_w, fc1_b, fc2_w, fc2_b, fc3_w, fc3_b
  float* stats;             // [4]
  int32_t off[7];           // start of each gradient tensor in a partial vector; off[6] = the four sums
  int32_t n_parts, np;
  double B;
  float l2_reg;
};

// Workgroups 0 .. gridDim.x - 2: sixteen consecutive gradient entries each (reduce16_entries), plus 2 l2_reg W on the weight
// tensors.  The last workgroup: the four sums and the three ||W||^2 (256 strided slices each, then a tree), and from them `stats`.
__global__ __launch_bounds__(256) void ppo_critic_reduce_kernel(const PpoCriticReduceArgs o) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  if (blockIdx.x + 1 < gridDim.x) {
    reduce16_store(o.partials, o.n_parts, o.np, o.off, o.grad, red, [&](int k, int j, double v) {
      return (k & 1) == 0 ? v + 2.0 * (double)o.l2_reg * (double)o.weight[k >> 1][j] : v;
    });
    return;
  }
  double sums[4], norm = 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) sums[q] = block_sum_column(o.partials + o.off[6] + q, o.n_parts, o.np, red);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int n = o.off[2 * k + 1] - o.off[2 * k];
    double mine = 0.0;
    for (int j = t; j < n; j += 256) { const double w = (double)o.weight[k][j]; mine += w * w; }
    norm += block_tree(red, mine);
  }
  if (t == 0) {
    const double mse = sums[0] / o.B, my = sums[2] / o.B;
    o.stats[0] = (float)(mse + (double)o.l2_reg * norm);
    o.stats[1] = (float)mse;
    o.stats[2] = (float)(sums[1] / o.B);
    const double var = sums[3] / o.B - my * my;
    o.stats[3] = (float)(var > 0.0 ? var : 0.0);
  }
}

}  // namespace qr
