// qr_shuffle.h — part of the gfx950 quadrotor step library (included by quadrotor_kernels.hip, after qr_noise.h).
// A keyed permutation of [0, n) (qr_shuffle): PPO's epoch shuffle with no sort, no state and no stored table.  out[i] = perm(first + i).
//
// perm(i) walks a balanced Feistel network on 2w bits (w the smallest integer in 1..16 with 4^w >= n) from x = i until the result is
// below n.  kShuffleRounds rounds, round r: (L, R) <- (R, L ^ F_r(R)), F_r(v) = shuffle_mix32(v + key[r]) >> (32 - w).  key[4k .. 4k + 3]
// are the raw Philox4x32-10 words of quad k of the noise stream (seed, draw, stream): noise_fill_kernel's counter, the words before they
// become floats.  A value depends on (seed, draw, stream, n, first + i) alone: not on the grid, the slice or another call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "quadrotor_hip.h"
#include "qr_rng.h"
#include "qr_noise.h"

namespace qr {

constexpr int kShuffleRounds = QR_SHUFFLE_ROUNDS;
constexpr int kShuffleBlock = 256;
constexpr int kShuffleGrid = kNoiseGrid;   // workgroups at the most by default (noise_fill_kernel's), then the threads stride on
static_assert(kShuffleRounds % 4 == 0 && kShuffleRounds <= kShuffleBlock * 4, "a quad of keys per thread of the first ones");
// the finaliser's two odd multipliers (a 32-bit multiply-xorshift hash with shifts 16, 15, 16)
constexpr uint32_t kShuffleMixM1 = QR_SHUFFLE_MIX_M1, kShuffleMixM2 = QR_SHUFFLE_MIX_M2;

struct ShuffleArgs {
  int64_t* out;
  const int64_t* draw_dev;   // null: `draw` below; else the draw number is *draw_dev (read only)
  int64_t draw;
  uint64_t seed;
  uint32_t n, first, count;  // first + count <= n < 2^32
  uint32_t stream, w;        // w: half the network's width in bits, 1..16
};

__device__ __forceinline__ uint32_t shuffle_mix32(uint32_t x) {
  x ^= x >> 16; x *= kShuffleMixM1;
  x ^= x >> 15; x *= kShuffleMixM2;
  return x ^ (x >> 16);
}

// One thread per output element, 8-byte stores.  The kShuffleRounds keys are the same for every element: the first kShuffleRounds / 4
// threads of a workgroup form one Philox quad each and leave it in LDS (32 bytes, the kernel's only LDS), and every thread reads the
// keys from there once, at one address per wave.  No atomics; no thread reads a word that another writes, and the counter word is
// only read.  The walk ends: the network is a bijection of [0, 4^w) and the start lies below n, so the cycle it follows returns there.
__global__ __launch_bounds__(kShuffleBlock) void shuffle_kernel(const ShuffleArgs o) {
  __shared__ uint32_t keys[kShuffleRounds];
  if (threadIdx.x < kShuffleRounds / 4) {
    const uint64_t draw = o.draw_dev ? (uint64_t)*o.draw_dev : (uint64_t)o.draw;
    // (quad k < 2^32: its high half is 0)
    uint32_t ctr[4] = {threadIdx.x, (uint32_t)(draw >> 32), (uint32_t)draw, 0x80000000u | 0x40000000u | o.stream};
    philox4x32_10(ctr, (uint32_t)o.seed, (uint32_t)(o.seed >> 32));
#pragma unroll
    for (int j = 0; j < 4; ++j) keys[4 * threadIdx.x + j] = ctr[j];
  }
  __syncthreads();
  uint32_t key[kShuffleRounds];
#pragma unroll
  for (int r = 0; r < kShuffleRounds; ++r) key[r] = keys[r];

  const uint32_t w = o.w, mask = (1u << w) - 1u, down = 32u - w;
  const uint64_t stride = (uint64_t)gridDim.x * kShuffleBlock;
  // (64-bit positions: count may lie within one stride of 2^32)
  for (uint64_t f = (uint64_t)blockIdx.x * kShuffleBlock + threadIdx.x; f < o.count; f += stride) {
    uint32_t x = o.first + (uint32_t)f;   // < n
    do {
      uint32_t L = x >> w, R = x & mask;
#pragma unroll
      for (int r = 0; r < kShuffleRounds; ++r) {
        const uint32_t t = L ^ (shuffle_mix32(R + key[r]) >> down);
        L = R; R = t;
      }
      x = (L << w) | R;
    } while (x >= o.n);
    o.out[f] = (int64_t)x;
  }
}

}  // namespace qr
