// qr_es.h — part of the gfx950 quadrotor step library (included by quadrotor_kernels.hip, after qr_noise.h).
// What surrounds the population evaluation in an evolution-strategy generation (qr_es_perturb, qr_es_gradient):
//   es_perturb_kernel   the antithetic population theta +- sigma eps around the base tensors, and the copies of the tensors that are
//                       not perturbed, in one launch
//   es_utility_kernel   fitness [P] -> the pair weights w_j = u_2j - u_2j+1 (centered ranks or standardised fitness) and the statistics
//   es_grad_kernel      grad[e] = -(sum_j w_j eps_j[e]) / (P sigma), eps regenerated from the key
//
// The perturbation stream.  Tensor i has n elements, Q = ceil(n / 4) quads and a stream id s < 2^30.  The draw of pair j for element e
// is element j * 4 Q + e of the qr_noise_fill stream (seed, draw = generation, stream = s, NORMAL, a = 0, b = 1): quad j * Q + e / 4,
// position e % 4 — normal4(z, seed, j * Q + e / 4, generation, 0x40000000 | s), and noise_fill_kernel's fmaf(1, z, 0) behind it.  So
// the eps of a generation is what qr_noise_fill writes into a [P / 2][4 Q] tensor under the same key, bit for bit, and it is never
// stored: both kernels regenerate it.  A value depends on (seed, generation, stream, j, e) alone: not on the tensor's place in the
// launch, the other tensors, the grid or a pointer's alignment.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "quadrotor_hip.h"
#include "qr_rng.h"
#include "qr_actor.h"
#include "qr_noise.h"

namespace qr {

constexpr int kEsSlots = QR_ES_MAX_TENSORS;
constexpr int kEsCopies = QR_ES_MAX_COPIES;
constexpr int kEsBlock = 256;
constexpr int kEsGrid = 1024;        // workgroups of the perturbation at the most (noise_fill_kernel's), then the threads stride on
constexpr int kEsGradGrid = 2048;    // waves of the estimator at the most (two per SIMD), then they stride on
constexpr int kEsTile = 1024;        // fitness keys per LDS tile of the rank count

// One quad of a stream: noise_fill_kernel's NORMAL slot with a = 0, b = 1 (the fused multiply-add turns a -0 into +0, as there).
__device__ __forceinline__ void es_eps4(float (&z)[4], uint64_t seed, uint64_t q, uint64_t generation, uint32_t stream) {
  normal4(z, seed, q, generation, 0x40000000u | stream);
#pragma unroll
  for (int i = 0; i < 4; ++i) z[i] = fmaf(1.0f, z[i], 0.0f);
}

// Four values to p, of which `left` >= 1 exist: one 16-byte store where the quad is whole and p is 16-byte aligned, else element by
// element (noise_fill_kernel's store, with its opaque copies against a merge of the two forms).
__device__ __forceinline__ void es_store4(float* p, const float (&x)[4], int64_t left) {
  if (left >= 4 && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
    typedef float quad_t __attribute__((ext_vector_type(4)));
    float v0 = x[0], v1 = x[1], v2 = x[2], v3 = x[3];
    asm volatile("" : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3));
    const quad_t v = {v0, v1, v2, v3};
    *reinterpret_cast<quad_t*>(p) = v;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < left) p[i] = x[i];
  }
}

// qend[k] = the flat pair-quad behind tensor k's last ((P / 2) * Q each); qend[k] = qend[15] = the launch's total (below 2^31) for
// k >= n_tensors - 1, so that an unused slot is never selected.
struct EsPerturbArgs {
  uint32_t qend[kEsSlots];
  const float* base[kEsSlots];
  float* out[kEsSlots];             // [P][count]
  uint32_t count[kEsSlots], quads[kEsSlots], stream[kEsSlots];
  const float* csrc[kEsCopies];     // the tensors that are copied to all P rows
  float* cdst[kEsCopies];
  uint32_t ccount[kEsCopies];
  int32_t n_copies;
  uint32_t P;
  float sigma;
  uint64_t seed;
  const int64_t* gen_dev;           // null: `gen` below; else the generation is *gen_dev (read only)
  int64_t gen;
};
static_assert(sizeof(EsPerturbArgs) <= 4096, "the descriptor must fit one kernarg segment");

// One thread owns one quad of one pair: flat index f -> tensor (a select chain over the sixteen offsets), then local = f - first =
// j * Q + qi, which is the stream's quad number itself.  One Philox call, the base quad read once, two stores: row 2j gets
// fl(theta + d), row 2j + 1 fl(theta - d) with d = fl(sigma * eps) — ActorPopulation.perturb's arithmetic.  The product is pinned in a
// register before the sums: the build contracts a visible product into the addition (-ffp-contract=fast), which would round once
// where the population rounds twice.  The tensor's members are read with the lane's own slot, as vector loads of the kernarg segment.
// No LDS, no atomics; no thread reads a word that another writes.
__global__ __launch_bounds__(kEsBlock) void es_perturb_kernel(const EsPerturbArgs o) {
  const uint64_t gen = o.gen_dev ? (uint64_t)*o.gen_dev : (uint64_t)o.gen;
  const uint32_t total = o.qend[kEsSlots - 1];
  const uint32_t tid = blockIdx.x * kEsBlock + threadIdx.x;
  const uint32_t stride = gridDim.x * kEsBlock;
  // (f + stride cannot wrap: total < 2^31 and stride <= 2^18)
  for (uint32_t f = tid; f < total; f += stride) {
    int slot = 0;
    uint32_t first = 0;
#pragma unroll
    for (int k = 0; k < kEsSlots - 1; ++k)
      if (f >= o.qend[k]) { slot = k + 1; first = o.qend[k]; }
    const uint32_t local = f - first;
    const uint32_t Q = o.quads[slot], n = o.count[slot];
    const uint32_t j = local / Q, qi = local - j * Q;
    const uint32_t e0 = qi << 2;
    const int64_t left = (int64_t)n - (int64_t)e0;   // elements of the tensor from this quad on: >= 1
    float z[4], d[4], th[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    es_eps4(z, o.seed, (uint64_t)local, gen, o.stream[slot]);
    const float* const b = o.base[slot] + e0;
    if (left >= 4 && (reinterpret_cast<uintptr_t>(b) & 15u) == 0) {
      const float4 v = *reinterpret_cast<const float4*>(b);
      th[0] = v.x; th[1] = v.y; th[2] = v.z; th[3] = v.w;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (i < left) th[i] = b[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) d[i] = o.sigma * z[i];
    asm volatile("" : "+v"(d[0]), "+v"(d[1]), "+v"(d[2]), "+v"(d[3]));
    float hi[4], lo[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { hi[i] = th[i] + d[i]; lo[i] = th[i] - d[i]; }
    float* const p = o.out[slot] + (int64_t)(2 * j) * n + e0;
    es_store4(p, hi, left);
    es_store4(p + n, lo, left);
  }
  for (int c = 0; c < o.n_copies; ++c) {
    const uint32_t n = o.ccount[c];
    const float* const src = o.csrc[c];
    float* const dst = o.cdst[c];
    const uint64_t all = (uint64_t)o.P * n;
    for (uint64_t i = tid; i < all; i += stride) dst[i] = src[i % n];
  }
}

struct EsUtilityArgs {
  const float* fitness;   // [P]
  double* w;              // [P / 2]
  double* stats;          // [QR_ES_STATS]
  int32_t P, shaping;
};

// The statistics of the fitness in float64, in index order, by ONE thread: mean = (sum of the values) / P, the first largest value
// (NaNs never compare larger; -inf and index 0 where nothing does), whether a value is non-finite and — with_std — the unbiased
// standard deviation from a second pass over (f - mean)^2.
struct EsFitnessStats { double mean, max, argmax, bad, std; };
__device__ __forceinline__ EsFitnessStats es_fitness_stats(const float* f, int P, bool with_std) {
  EsFitnessStats s{0.0, -__builtin_inf(), 0.0, 0.0, 0.0};
  double sum = 0.0;
  for (int i = 0; i < P; ++i) {
    const double x = (double)f[i];
    sum += x;
    if (x > s.max) { s.max = x; s.argmax = (double)i; }
    if (!(fabs(x) <= 1.7976931348623157e308)) s.bad = 1.0;
  }
  s.mean = sum / (double)P;
  if (with_std) {
    double sq = 0.0;
    for (int i = 0; i < P; ++i) {
      const double dx = (double)f[i] - s.mean;
      sq += dx * dx;
    }
    s.std = sqrt(sq / (double)(P - 1));
  }
  return s;
}

// One thread per policy, ceil(P / 256) workgroups; P is even, so the two members of a pair are neighbouring lanes of one wave and the
// even one writes the pair's weight.
//   CENTERED_RANK  key_i = f_i, or -inf for a NaN.  Every thread counts, over all P keys out of LDS tiles (each lane reads the same
//                  words: broadcasts), the keys below its own and the keys equal to it, in integers:
//                  rank_i = less + (equal - 1) / 2, u_i = rank_i / (P - 1) - 1/2.  The padding of the last tile is NaN, which counts
//                  as neither.  rank_i is a half-integer below 2^13: exact, so u_i is one division and one subtraction in float64.
//   STANDARDIZE    w_j = (f_2j - f_2j+1) / (std + 1e-8): u_2j - u_2j+1 with the mean cancelled, the difference of two float32
//                  numbers formed in float64.  Thread 0 of every workgroup forms mean and std for itself (index order).
//                  A non-finite fitness: every weight is zero.
// stats: by thread 0 of workgroup 0.
__global__ __launch_bounds__(kEsBlock) void es_utility_kernel(const EsUtilityArgs a) {
  __shared__ __attribute__((aligned(16))) float tile[kEsTile];
  __shared__ double shared_den;
  const int P = a.P;
  const int i = blockIdx.x * kEsBlock + threadIdx.x;
  const bool active = i < P;
  const float fi = active ? a.fitness[i] : 0.0f;
  double u = 0.0;
  if (a.shaping == QR_ES_CENTERED_RANK) {
    const float key = fi != fi ? -__builtin_inff() : fi;
    int less = 0, equal = 0;
    for (int t0 = 0; t0 < P; t0 += kEsTile) {
      __syncthreads();
      for (int k = threadIdx.x; k < kEsTile; k += kEsBlock) {
        const float x = t0 + k < P ? a.fitness[t0 + k] : __builtin_nanf("");
        tile[k] = (t0 + k < P && x != x) ? -__builtin_inff() : x;
      }
      __syncthreads();
      const int nk = P - t0 < kEsTile ? (P - t0 + 3) & ~3 : kEsTile;   // (whole quads: the tile's tail holds NaNs)
      for (int k = 0; k < nk; k += 4) {
        const float4 x = *reinterpret_cast<const float4*>(&tile[k]);
        less += (x.x < key) + (x.y < key) + (x.z < key) + (x.w < key);
        equal += (x.x == key) + (x.y == key) + (x.z == key) + (x.w == key);
      }
    }
    const double rank = (double)less + 0.5 * (double)(equal - 1);
    u = rank / (double)(P - 1) - 0.5;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      const EsFitnessStats s = es_fitness_stats(a.fitness, P, false);
      a.stats[0] = s.mean; a.stats[1] = s.max; a.stats[2] = s.argmax; a.stats[3] = s.bad;
    }
  } else {
    if (threadIdx.x == 0) {
      const EsFitnessStats s = es_fitness_stats(a.fitness, P, true);
      shared_den = s.bad != 0.0 ? 0.0 : s.std + 1e-8;   // (0: the non-finite mark)
      if (blockIdx.x == 0) { a.stats[0] = s.mean; a.stats[1] = s.max; a.stats[2] = s.argmax; a.stats[3] = s.bad; }
    }
    __syncthreads();
    u = (double)fi;
  }
  const double other = __shfl_down(u, 1);
  if (active && (threadIdx.x & 1) == 0) {
    double w = u - other;
    if (a.shaping != QR_ES_CENTERED_RANK) w = shared_den != 0.0 ? w / shared_den : 0.0;
    a.w[i >> 1] = w;
  }
}

// qend[k] = the flat quad behind tensor k's last (Q each), padded as above.
struct EsGradArgs {
  uint32_t qend[kEsSlots];
  float* grad[kEsSlots];            // [count]
  uint32_t count[kEsSlots], quads[kEsSlots], stream[kEsSlots];
  const double* w;                  // [half]
  uint32_t half;                    // P / 2
  double den;                       // P * sigma (exact in float64)
  uint64_t seed;
  const int64_t* gen_dev;
  int64_t gen;
};
static_assert(sizeof(EsGradArgs) <= 4096, "the descriptor must fit one kernarg segment");

// One wave owns one quad of one tensor (the slot is wave-uniform): lane l regenerates the quad's draws of the pairs l, l + 64, ... in
// that order and adds w_j * (double)eps to four float64 sums, a fixed shuffle tree (lane l takes lane l + off; gae_rule_kernel's)
// folds the 64 lanes, and lane 0 rounds -(sum / (P sigma)) to float32 once.  A quad's sum is formed by one wave in one order: the
// same bits from call to call and for any grid.  No floating-point atomics, no LDS; eps is never read from memory.
__global__ __launch_bounds__(64) void es_grad_kernel(const EsGradArgs o) {
  const uint64_t gen = o.gen_dev ? (uint64_t)*o.gen_dev : (uint64_t)o.gen;
  const uint32_t total = o.qend[kEsSlots - 1];
  const uint32_t lane = threadIdx.x;
  for (uint32_t f = blockIdx.x; f < total; f += gridDim.x) {
    int slot = 0;
    uint32_t first = 0;
#pragma unroll
    for (int k = 0; k < kEsSlots - 1; ++k)
      if (f >= o.qend[k]) { slot = k + 1; first = o.qend[k]; }
    const uint32_t qi = f - first;
    const uint32_t Q = o.quads[slot], stream = o.stream[slot];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (uint32_t j = lane; j < o.half; j += 64) {
      float z[4];
      es_eps4(z, o.seed, (uint64_t)j * Q + qi, gen, stream);
      const double wj = o.w[j];
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] += wj * (double)z[c];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] += __shfl_down(acc[c], off);
    }
    if (lane == 0) {
      float g[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) g[c] = (float)(-(acc[c] / o.den));
      es_store4(o.grad[slot] + ((int64_t)qi << 2), g, (int64_t)o.count[slot] - ((int64_t)qi << 2));
    }
  }
}

}  // namespace qr
