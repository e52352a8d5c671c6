// qr_optim.h — part of the gfx950 quadrotor step library (included by quadrotor_kernels.hip, after qr_ppo_critic.h).
// What follows a gradient launch in PPO.train (algos/ppo/ppo.py:185-190, 209-214): clip_grad_norm_, AdamW.step() and
// CosineAnnealingWarmRestarts.step() for up to eight independent parameter groups in one launch: adamw_step_kernel (qr_adamw_step).
// adamw_polyak_kernel (qr_adamw_polyak_step) is the same step for groups of up to sixteen tensors — a twin critic's twelve under ONE
// clip, as TD3.train / SAC.train step it (td3.py:166-171, sac.py:165-170) — followed, in the same launch, by the soft update of the
// group's target tensors (td3.py:207-211) and, for SAC's one-entry log_alpha group, by alpha = exp(log_alpha) (sac.py:213).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "quadrotor_hip.h"

namespace qr {

constexpr int kAdamWGroups = 8, kAdamWTensors = 8;
constexpr int kAdamWMaxEntries = 65536;  // per group: 256 entries per thread at the most

// One group = what one torch.optim.AdamW instance holds here.  off[k] = the flat entry at which tensor k starts, off[k] = off[8] =
// the group's total for k >= n_tensors, so that an unused slot is never selected.
struct AdamWGroupArgs {
  float* param[kAdamWTensors];
  const float* grad[kAdamWTensors];
  int32_t off[kAdamWTensors + 1];
  int32_t reserved0;
  float *exp_avg, *exp_avg_sq;  // [off[8]] each, the tensors back to back
  int64_t* step;
  float* stats;                 // [4] or NULL
  double lr, eta_min;
  int64_t t0;
  float beta1, beta2, eps, weight_decay, max_norm;
  int32_t reserved1;
};

struct AdamWArgs {
  AdamWGroupArgs g[kAdamWGroups];
};

// One workgroup of 256 threads per group; groups never interact.  In order: the 2-norm of all of the group's gradient entries
// (per-thread strided sums of squares in float64, then an LDS tree: the order depends on the sizes alone), the step's scalars in
// float64 on one thread (the schedule's rate, the clip coefficient, the bias corrections), the update of every entry in float32 as
// torch's AdamW forms it, the step counter.  A thread reads its own group's descriptor of the kernarg segment and nothing else.
// The gradient tensors are read only.
__global__ __launch_bounds__(256) void adamw_step_kernel(const AdamWArgs o) {
  __shared__ double red[256];
  __shared__ float sc[6];
  const AdamWGroupArgs& d = o.g[blockIdx.x];
  const int t = threadIdx.x, n = d.off[kAdamWTensors];

  // the tensor of flat entry e, from the offsets (as ppo_reduce_kernel locates its destination)
  auto locate = [&](int e, float*& p, const float*& g) {
    int base = 0;
    p = d.param[0]; g = d.grad[0];
#pragma unroll
    for (int k = 1; k < kAdamWTensors; ++k)
      if (e >= d.off[k]) { p = d.param[k]; g = d.grad[k]; base = d.off[k]; }
    p += e - base; g += e - base;
  };

  double mine = 0.0;
  for (int e = t; e < n; e += 256) {
    float* p; const float* g;
    locate(e, p, g);
    const double x = (double)*g;
    mine += x * x;
  }
  red[t] = mine;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }

  int64_t step = 0;
  double total_norm = 0.0, lr_t = 0.0, clip64 = 1.0;
  if (t == 0) {
    total_norm = sqrt(red[0]);
    step = *d.step + 1;
    lr_t = d.lr;
    if (d.t0 > 0) lr_t = d.eta_min + (d.lr - d.eta_min) * (1.0 + cospi((double)((step - 1) % d.t0) / (double)d.t0)) * 0.5;
    if (d.max_norm >= 0.0f) {
      clip64 = (double)d.max_norm / (total_norm + 1e-6);
      clip64 = clip64 > 1.0 ? 1.0 : clip64;  // (a NaN norm stays a NaN coefficient, as torch.clamp leaves it)
    }
    // beta^step by squaring: at most 63 float64 products
    double p1 = 1.0, p2 = 1.0, b1 = (double)d.beta1, b2 = (double)d.beta2;
    for (int64_t k = step; k > 0; k >>= 1) {
      if (k & 1) { p1 *= b1; p2 *= b2; }
      b1 *= b1; b2 *= b2;
    }
    const double bc1 = 1.0 - p1, bc2 = 1.0 - p2;
    sc[0] = (float)clip64;
    sc[1] = (float)(1.0 - lr_t * (double)d.weight_decay);
    sc[2] = (float)(lr_t / bc1);
    sc[3] = (float)sqrt(bc2);
    sc[4] = (float)(1.0 - (double)d.beta1);
    sc[5] = (float)(1.0 - (double)d.beta2);
  }
  __syncthreads();
  const float clip = sc[0], decay = sc[1], step_size = sc[2], bc2_sqrt = sc[3], omb1 = sc[4], omb2 = sc[5];
  const float beta1 = d.beta1, beta2 = d.beta2, eps = d.eps;
  for (int e = t; e < n; e += 256) {
    float* p; const float* gp;
    locate(e, p, gp);
    const float g = clip * *gp;
    const float w = *p * decay;
    const float m = beta1 * d.exp_avg[e] + omb1 * g;
    const float v = beta2 * d.exp_avg_sq[e] + omb2 * (g * g);
    d.exp_avg[e] = m;
    d.exp_avg_sq[e] = v;
    *p = w - step_size * (m / (sqrtf(v) / bc2_sqrt + eps));
  }
  if (t == 0) {
    *d.step = step;
    if (d.stats) {
      d.stats[0] = (float)total_norm; d.stats[1] = (float)clip64; d.stats[2] = (float)lr_t; d.stats[3] = (float)step;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// qr_adamw_polyak_step
// ------------------------------------------------------------------------------------------------------------------
constexpr int kPolyakTensors = 16;
constexpr int kPolyakGroups = 7;  // 7 x 552 bytes = 3 864: eight descriptors (4 416 bytes) would pass the 4 096 bytes of a kernarg segment

// AdamWGroupArgs with sixteen tensor slots, a target per slot (NULL: none) and the exp output.  off[k] = off[16] for k >= n_tensors.
struct AdamWPolyakGroupArgs {
  float* param[kPolyakTensors];
  const float* grad[kPolyakTensors];
  float* target[kPolyakTensors];
  int32_t off[kPolyakTensors + 1];
  int32_t reserved0;
  float *exp_avg, *exp_avg_sq;
  int64_t* step;
  float* stats;    // [4] or NULL
  float* exp_out;  // [1] or NULL (only where off[16] == 1)
  double lr, eta_min;
  int64_t t0;
  float beta1, beta2, eps, weight_decay, max_norm;
  float tau, omt;  // float32(tau), float32(1.0 - tau) with the subtraction in double, as SoftUpdateArgs holds them
};

struct AdamWPolyakArgs {
  AdamWPolyakGroupArgs g[kPolyakGroups];
};
static_assert(sizeof(AdamWPolyakArgs) <= 4096, "the descriptors must fit one kernarg segment");

// soft_update_kernel's `rounded` (qr_td3_actor.h, included after this file), restated: a product that the sum after it cannot be
// fused with, whatever -ffp-contract says.
__device__ __forceinline__ float polyak_rounded(float v) {
  asm volatile("" : "+v"(v));
  return v;
}

// adamw_step_kernel for groups of up to sixteen tensors: the norm reduction, the scalar thread and the per-entry update are that
// kernel's, in its order and with its strides, so that a group both kernels take gets the same bits from either.  Then the thread
// that wrote entry e of param[k] forms target[k][e] from the value it has just stored and the old target, in soft_update_kernel's
// expression (two products and a sum, each rounded on its own), and thread 0 — which wrote entry 0 — stores exp of a one-entry
// group's new value.  No thread reads a word that another thread writes; a target tensor is touched by its parameter's thread alone.
__global__ __launch_bounds__(256) void adamw_polyak_kernel(const AdamWPolyakArgs o) {
  __shared__ double red[256];
  __shared__ float sc[6];
  const AdamWPolyakGroupArgs& d = o.g[blockIdx.x];
  const int t = threadIdx.x, n = d.off[kPolyakTensors];

  // the tensor of flat entry e and the entry's position in it
  auto locate = [&](int e, int& base) {
    int slot = 0;
    base = 0;
#pragma unroll
    for (int k = 1; k < kPolyakTensors; ++k)
      if (e >= d.off[k]) { slot = k; base = d.off[k]; }
    return slot;
  };
  // (a select chain over the kernarg's pointers: a runtime index into them would move the descriptor to scratch)
  auto pick = [&](int slot, float*& p, const float*& g, float*& tg) {
    p = d.param[0]; g = d.grad[0]; tg = d.target[0];
#pragma unroll
    for (int k = 1; k < kPolyakTensors; ++k)
      if (slot == k) { p = d.param[k]; g = d.grad[k]; tg = d.target[k]; }
  };

  double mine = 0.0;
  for (int e = t; e < n; e += 256) {
    float *p, *tg; const float* g;
    int base;
    pick(locate(e, base), p, g, tg);
    const double x = (double)g[e - base];
    mine += x * x;
  }
  red[t] = mine;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }

  int64_t step = 0;
  double total_norm = 0.0, lr_t = 0.0, clip64 = 1.0;
  if (t == 0) {
    total_norm = sqrt(red[0]);
    step = *d.step + 1;
    lr_t = d.lr;
    if (d.t0 > 0) lr_t = d.eta_min + (d.lr - d.eta_min) * (1.0 + cospi((double)((step - 1) % d.t0) / (double)d.t0)) * 0.5;
    if (d.max_norm >= 0.0f) {
      clip64 = (double)d.max_norm / (total_norm + 1e-6);
      clip64 = clip64 > 1.0 ? 1.0 : clip64;  // (a NaN norm stays a NaN coefficient, as torch.clamp leaves it)
    }
    double p1 = 1.0, p2 = 1.0, b1 = (double)d.beta1, b2 = (double)d.beta2;
    for (int64_t k = step; k > 0; k >>= 1) {
      if (k & 1) { p1 *= b1; p2 *= b2; }
      b1 *= b1; b2 *= b2;
    }
    const double bc1 = 1.0 - p1, bc2 = 1.0 - p2;
    sc[0] = (float)clip64;
    sc[1] = (float)(1.0 - lr_t * (double)d.weight_decay);
    sc[2] = (float)(lr_t / bc1);
    sc[3] = (float)sqrt(bc2);
    sc[4] = (float)(1.0 - (double)d.beta1);
    sc[5] = (float)(1.0 - (double)d.beta2);
  }
  __syncthreads();
  const float clip = sc[0], decay = sc[1], step_size = sc[2], bc2_sqrt = sc[3], omb1 = sc[4], omb2 = sc[5];
  const float beta1 = d.beta1, beta2 = d.beta2, eps = d.eps;
  for (int e = t; e < n; e += 256) {
    float *p, *tg; const float* gp;
    int base;
    pick(locate(e, base), p, gp, tg);
    const int i = e - base;
    const float g = clip * gp[i];
    const float w = p[i] * decay;
    const float m = beta1 * d.exp_avg[e] + omb1 * g;
    const float v = beta2 * d.exp_avg_sq[e] + omb2 * (g * g);
    d.exp_avg[e] = m;
    d.exp_avg_sq[e] = v;
    const float fresh = w - step_size * (m / (sqrtf(v) / bc2_sqrt + eps));
    p[i] = fresh;
    if (tg) tg[i] = polyak_rounded(__fmul_rn(d.tau, fresh)) + polyak_rounded(__fmul_rn(d.omt, tg[i]));
    if (e == 0 && d.exp_out) *d.exp_out = (float)exp((double)fresh);  // (e == 0 is thread 0's first entry; n == 1 here)
  }
  if (t == 0) {
    *d.step = step;
    if (d.stats) {
      d.stats[0] = (float)total_norm; d.stats[1] = (float)clip64; d.stats[2] = (float)lr_t; d.stats[3] = (float)step;
    }
  }
}

}  // namespace qr
