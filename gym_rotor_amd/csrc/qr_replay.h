// qr_replay.h — part of the gfx950 quadrotor step library (included by quadrotor_kernels.hip, in this order).
// The data side of a TD3 / SAC iteration: the replay buffer's append and its minibatch indices.
//   replay_add_kernel (qr_replay_add)        one horizon of a RolloutStorage into the ring of a flat transition buffer: all agents, all
//                                            five tensors, one launch, no temporaries
//   replay_add_rule_kernel (qr_replay_add_rule)  the same append with the reference's time-limit "solved" rule in its done segment
//   replay_sample_kernel (qr_replay_sample)  B pairwise distinct rows below n in O(B): a keyed Feistel permutation of [0, n), integer only
//   replay_advance_kernel                    the opt-in device counters (count, current_size, draw), advanced by ONE thread in a launch of
//                                            its own behind the kernel that read them: no workgroup reads a word that a workgroup of the
//                                            same launch writes, and nothing waits on a launch-end atomic
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "qr_rng.h"

namespace qr {

// ------------------------------------------------------------------------------------------------------------------
// qr_replay_add
// ------------------------------------------------------------------------------------------------------------------
constexpr int kReplayTile = 64;        // transitions per tile: one workgroup moves a tile's rows of ONE tensor, then strides on
constexpr int kReplayCols = 2048;      // workgroups per tensor (grid-stride over the tiles)
constexpr int kReplaySegments = 5;     // obs, obs_next, act, rwd, done
constexpr int kReplayMaxWidth = 4096;  // widest row: keeps magic-number division exact (l * (magic * w - 2^32) < 2^32 for l < 64 w)

struct ReplayAddArgs {
  // the horizon, as RolloutStorage holds it
  const float *obs0, *obs1;            // [T + 1][N][D_k]
  const float *final0, *final1;        // [T][N][D_k], or both null
  const float* action;                 // [T][N][action_row]
  const float* reward;                 // [T][N][n_agents]
  const uint8_t* done;                 // [T][N][n_agents]
  const uint8_t* truncated;            // [T][N], or null
  // the buffer, [capacity][width] each
  float *b_obs0, *b_obs1, *b_next0, *b_next1, *b_act0, *b_act1, *b_rwd0, *b_rwd1, *b_done0, *b_done1;
  const int64_t* state;                // null: `count` below; else count = state[0]
  int64_t count, capacity, rows;       // rows = T * N
  int64_t next0, next1;                // N * D_k: from obs[t] to obs[t + 1]
  int32_t D0, D1, A0, A1, col0, col1, action_row, n_agents;
  uint32_t mD0, mD1, mA0, mA1;         // ceil(2^32 / width) for width >= 2
};

// Workgroup row blockIdx.y owns one tensor of one agent (5 k + segment); blockIdx.x strides over 64-transition tiles.  Inside a tile the
// thread index runs over the tile's ELEMENTS in buffer order, so a wave's 64 lanes write 256 consecutive bytes of the buffer (a tile's
// rows are contiguous in the ring except across its wrap) and read 256 consecutive bytes of obs / final_obs; the action, reward and done
// rows are read with the stride the storage gives them.  Element offsets are 64-bit; the offset inside a tile is 32-bit and is split
// into (row, column) by a multiply-high.
//
// The kernel exists twice, from ONE text (qr_replay_walk.h, included into both bodies): replay_add_kernel, and replay_add_rule_kernel
// (kRule), whose done segment is written by the reference's time-limit rule (main.py:169-173) instead of the agent's own flag: on a
// transition whose `truncated` is set, done = the agent's error is within tolerance in the observation the transition stores as
// obs_next, and its reward is not the crash reward; elsewhere the own flag.  That segment then reads, per transition and still in
// transition order (a wave writes 256 consecutive bytes of done), the truncated byte and — on a time-limit row — one reward word
// and 3 (agent 0: ex) or 1 (agent 1: eb1) observation words.  The comparisons are made in double on the float32 words, so
// tests/replay_rule_ref.py gives the same bits.  Every other segment is the same code.  (An inlined function template over the
// flag compiles replay_add_kernel to other instructions than it had; the shared text leaves it as it was.)
struct ReplayRule {
  double x_lim, pos_tol, rot_tol;
};

constexpr double kReplayPi = 3.141592653589793;   // the double nearest pi (np.pi)

__global__ __launch_bounds__(256) void replay_add_kernel(const ReplayAddArgs a) {
  constexpr bool kRule = false;
  const ReplayRule rule{};
#include "qr_replay_walk.h"
}

// The same launch with the time-limit rule in its done segment (qr_replay_add_rule).  `truncated` and `reward` are not null here,
// and agent 0's observation has at least three words.
struct ReplayAddRuleArgs {
  ReplayAddArgs add;
  ReplayRule rule;
};

__global__ __launch_bounds__(256) void replay_add_rule_kernel(const ReplayAddRuleArgs ra) {
  constexpr bool kRule = true;
  const ReplayAddArgs& a = ra.add;
  const ReplayRule& rule = ra.rule;
#include "qr_replay_walk.h"
}

// ------------------------------------------------------------------------------------------------------------------
// qr_replay_sample
// ------------------------------------------------------------------------------------------------------------------
constexpr int kReplayRounds = 6;

struct ReplaySampleArgs {
  int64_t* index;          // [batch]
  int32_t* status;         // null, or one word: set to 1 where a walk did not end (it always ends: see below)
  const int64_t* state;    // null: n, draw below; else n = state[1], draw = state[2]
  int64_t n, batch;
  uint64_t seed, draw;
};

// One pass of the balanced Feistel network on 2 h bits: (L, R) -> (R, L xor (F & mask)), six times, F = word 0 of Philox4x32-10 with the
// counter (R, round, draw_lo, draw_hi) under the key (seed_lo, seed_hi).  A permutation of [0, 4^h) whatever F is.
__device__ __forceinline__ uint32_t replay_feistel(uint32_t x, int h, uint32_t mask, uint64_t seed, uint64_t draw) {
  uint32_t L = x >> h, R = x & mask;
#pragma unroll 1
  for (int r = 0; r < kReplayRounds; ++r) {
    uint32_t ctr[4] = {R, (uint32_t)r, (uint32_t)draw, (uint32_t)(draw >> 32)};
    philox4x32_10(ctr, (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint32_t t = L ^ (ctr[0] & mask);
    L = R; R = t;
  }
  return (L << h) | R;   // (h = 16: L << 16 keeps all of L, which is below 2^16)
}

// index[j] = the image of j under the permutation of [0, n) that cycle-walking makes of the network: apply it until the value falls below
// n.  The walk starts at j < n and follows j's cycle in a permutation of 4^h < 4 n points, so it returns below n after at most 4^h
// steps (j itself closes the cycle); the loop is capped there all the same, and a capped walk stores 0 and raises *status.
__global__ __launch_bounds__(256) void replay_sample_kernel(const ReplaySampleArgs a) {
  const int64_t n = a.state ? a.state[1] : a.n;
  const uint64_t draw = a.state ? (uint64_t)a.state[2] : a.draw;
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.batch) return;
  if (n < 1 || n > 0x7FFFFFFFll || j >= n) {   // (device counters that do not admit this batch)
    a.index[j] = 0;
    if (a.status) *a.status = 1;
    return;
  }
  const int bits = 64 - __clzll((unsigned long long)(n - 1) | 1ull) - (n == 1);   // bit_length(n - 1)
  const int h = bits <= 2 ? 1 : (bits + 1) >> 1;
  const uint32_t mask = (1u << h) - 1u;
  const uint64_t cap = 1ull << (2 * h);
  uint32_t x = (uint32_t)j;
  uint64_t it = 0;
  do {
    x = replay_feistel(x, h, mask, a.seed, draw);
  } while (x >= (uint64_t)n && ++it < cap);
  const bool ok = x < (uint64_t)n;
  a.index[j] = ok ? (int64_t)x : 0;
  if (!ok && a.status) *a.status = 1;
}

// The device counters after one append of `rows` transitions and / or `draws` minibatches: the reference's ring rule, in one thread.
__global__ __launch_bounds__(64) void replay_advance_kernel(int64_t* state, int64_t rows, int64_t capacity, int64_t draws) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (rows > 0) {
    const int64_t count = state[0], size = state[1];
    if (count >= 0 && count < capacity) {
      const int64_t c = count + rows, s = size + rows;
      state[0] = c >= capacity ? c - capacity : c;
      state[1] = s < capacity ? s : capacity;
    }
  }
  if (draws > 0) state[2] = state[2] + draws;
}

}  // namespace qr
