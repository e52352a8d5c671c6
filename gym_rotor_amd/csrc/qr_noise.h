// qr_noise.h — part of the gfx950 quadrotor step library (included by quadrotor_kernels.hip, after qr_actor.h).
// The library's own noise source (qr_noise_fill): every random tensor an off-policy iteration consumes — up to sixteen of them, standard
// normal or uniform in (-1, 1), each scaled and shifted — filled in ONE launch from a counter-based stream.
//
// The stream.  Element e of a slot is position e % 4 of quad q = e / 4, and the quad's four words are Philox4x32-10 under the key
// (seed_lo, seed_hi) with the counter
//     { (uint32)q, (uint32)(q >> 32) ^ (uint32)(draw >> 32), (uint32)draw, 0x80000000 | 0x40000000 | stream }
// — normal4's layout (qr_actor.h) with gid = q, step = draw, block = 0x40000000 | stream.  Bit 30 keeps it apart from the rollout's
// blocks 0 and 1, the top bit from the reset stream and from replay_feistel's counters (whose fourth word is a draw number's high half:
// distinct as long as draws stay below 2^63).  NORMAL is normal4 itself on those words; UNIFORM is Draws::sym's expression on each word.
// A value depends on (seed, draw, stream, e, kind, a, b) alone: not on the slot's place in the launch, the other slots, the grid or the
// pointer's alignment.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "quadrotor_hip.h"
#include "qr_rng.h"
#include "qr_actor.h"

namespace qr {

constexpr int kNoiseSlots = QR_NOISE_MAX_SLOTS;
constexpr int kNoiseBlock = 256;
constexpr int kNoiseGrid = 1024;   // workgroups at the most: 2^18 quads in flight (four waves per SIMD), then the threads stride on

// qend[k] = the flat quad behind slot k's last; qend[k] = qend[15] = the launch's total (below 2^31) for k >= n_slots - 1, so that an
// unused slot is never selected.
struct NoiseArgs {
  uint32_t qend[kNoiseSlots];
  float* out[kNoiseSlots];
  int64_t count[kNoiseSlots];
  float a[kNoiseSlots], b[kNoiseSlots];
  uint32_t kind[kNoiseSlots], stream[kNoiseSlots];
  uint64_t seed;
  const int64_t* draw_dev;   // null: `draw` below; else the draw number is *draw_dev (read only)
  int64_t draw;
};
static_assert(sizeof(NoiseArgs) <= 4096, "the descriptor must fit one kernarg segment");

// One thread owns one quad: one Philox call, at most four stores.  The quad's slot comes from a select chain over the kernarg's sixteen
// quad offsets, read with constant indices.  The slot's members — 42 more words per slot, which a second select chain would have to
// hold in SGPRs all at once (it spilled 189 of them into VGPR lanes) — are read per slot instead: the wave takes the slots of its
// lanes one after the other (nearly always there is one), each as a wave-uniform index into the kernarg segment: six loads at one
// address per wave, issued together ahead of the Philox rounds, and the descriptor stays out of scratch (the compiler issues them
// as vector loads: it does not scalarise a load inside this loop).  A full quad at a 16-byte aligned address goes out as one 16-byte store;
// a slot whose pointer is not 16-byte aligned, and a slot's last, partial quad, element by element.  No LDS, no atomics; no thread
// reads a word that another writes, and the counter word is only read.
__global__ __launch_bounds__(kNoiseBlock) void noise_fill_kernel(const NoiseArgs o) {
  const uint64_t draw = o.draw_dev ? (uint64_t)*o.draw_dev : (uint64_t)o.draw;
  const uint32_t total = o.qend[kNoiseSlots - 1];
  const uint32_t stride = gridDim.x * kNoiseBlock;
  // (f + stride cannot wrap: total < 2^31 and stride <= 2^18)
  for (uint32_t f = blockIdx.x * kNoiseBlock + threadIdx.x; f < total; f += stride) {
    int slot = 0;
    uint32_t base = 0;
#pragma unroll
    for (int k = 0; k < kNoiseSlots - 1; ++k)
      if (f >= o.qend[k]) { slot = k + 1; base = o.qend[k]; }
    const uint64_t q = (uint64_t)(f - base);

    bool todo = true;
    while (todo) {
      // (the lanes compare with an opaque copy of the first lane's slot: were `slot == s` visible, the compiler would index with
      //  the lane's own slot again, per lane and through vector loads of the kernarg segment)
      const int s = __builtin_amdgcn_readfirstlane(slot);
      int mine = s;
      asm volatile("" : "+v"(mine));
      if (slot == mine) {
        todo = false;
        const float a = o.a[s], b = o.b[s];
        float* const p = o.out[s] + (q << 2);
        const int64_t left = o.count[s] - (int64_t)(q << 2);   // elements of the slot from this quad on: >= 1
        const uint32_t block = 0x40000000u | o.stream[s];
        float z[4];
        if (o.kind[s] == QR_NOISE_NORMAL) {
          normal4(z, o.seed, q, draw, block);
        } else {
          uint32_t ctr[4] = {(uint32_t)q, (uint32_t)(q >> 32) ^ (uint32_t)(draw >> 32), (uint32_t)draw, 0x80000000u | block};
          philox4x32_10(ctr, (uint32_t)o.seed, (uint32_t)(o.seed >> 32));
#pragma unroll
          for (int i = 0; i < 4; ++i) z[i] = fmaf((float)(ctr[i] >> 8), 0x1p-23f, 0x1p-24f - 1.0f);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) z[i] = fmaf(b, z[i], a);
        if (left >= 4 && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
          // (opaque copies: the element stores below must not be merged with this one, which split it into 12 + 4 bytes)
          typedef float quad_t __attribute__((ext_vector_type(4)));
          float v0 = z[0], v1 = z[1], v2 = z[2], v3 = z[3];
          asm volatile("" : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3));
          const quad_t v = {v0, v1, v2, v3};
          *reinterpret_cast<quad_t*>(p) = v;
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (i < left) p[i] = z[i];
        }
      }
    }
  }
}

}  // namespace qr
