// qr_critic.h — part of the gfx950 quadrotor step library (included by quadrotor_kernels.hip, after qr_actor.h).
// The reference's MLP critics (MLP_Critic / MLP_Critic_CTDE, algos/ppo/ppo_mlp.py:64-126) for a whole PPO horizon:
// critic_kernel (qr_critic_values, qr_critic_next_values).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "quadrotor_hip.h"
#include "qr_actor.h"

namespace qr {

struct CriticArgs {
  const float *fc1_w, *fc1_b, *fc2_w, *fc2_b, *fc3_w, *fc3_b;
  const float *rows0, *rows1;        // [n_rows][in0], [n_rows][in1]: obs rows (values) or final_obs rows (next values)
  const uint8_t *done, *truncated;   // next values only: [n_rows][n_agents], [n_rows] or NULL
  const float* value;                // next values only: [T+1][N] at element stride `stride`
  float* out;                        // value (values) or next_value (next values), element stride `stride`
  int64_t n_rows;                    // rows (values) or T * N (next values)
  int64_t n_envs;                    // next values: N, the distance from (t, n) to (t + 1, n)
  int32_t in0, in1, hidden, stride, n_agents;
};

constexpr int kCriticIn = 24;  // padded input width = row stride of the LDS tile

// v = fc3(tanh(fc2(tanh(fc1(x))))) for the 64 rows of an LDS tile, hidden width up to 64, on v_mfma_f32_16x16x4_f32 (exact f32)
// as the transposed GEMMs  H^T[64 x 64 rows] = W[64 x K] . X^T[K x 64]: ActorMfma's lane map (qr_actor.h) widened to four
// 16-unit hidden blocks.  The weights are the A operands and stay in registers for the whole launch (24 + 64), zero past
// the real sizes — exact, since tanh(0) = 0 and a padded unit's weights and bias are 0.
//   lane l: c = l & 15, g = l >> 4.   A: lane supplies A[c][k = g].  B: B[k = g][c].  D: lane holds D[4 g + r][c], r = 0..3.
//   layer 1: hidden block hb, row block b, k-step s: A = W1[16 hb + c][4 s + g], B = X[row 16 b + c][4 s + g] from the tile,
//            D = h1[hb][b][r] = H1[16 hb + 4 g + r][row 16 b + c].
//   layer 2: k-step (hb, r) is given the hidden units 16 hb + 4 g + r, so the lane's own tanh(h1[hb][b][r]) IS its B operand
//            and A = W2[16 ho + c][16 hb + 4 g + r]: no data moves between the layers.
//   layer 3 (64 -> 1): the lane's partial dot over its 16 hidden units on the VALU, then the transpose-reduce over the four
//            16-lane rows of ActorMfma::heads: lane (g, c) ends with the value of row 16 g + c — lane l, row l of the tile.
// The four row blocks go through in two halves: 2 x 32 accumulator registers live instead of 2 x 64, which keeps the kernel
// at two waves per SIMD, so that one wave's tanh (VALU) runs under the other's MFMAs.
struct CriticMfma {
  float a1[4][6], a2[4][4][4], w3[4][4], bias1[4][4], bias2[4][4], bias3;

  __device__ __forceinline__ void load(const CriticArgs& p, int lane) {
    const int c = lane & 15, g = lane >> 4, D = p.in0 + p.in1, H = p.hidden;
#pragma unroll
    for (int hb = 0; hb < 4; ++hb) {
      const int row = 16 * hb + c;
#pragma unroll
      for (int s = 0; s < 6; ++s) a1[hb][s] = (row < H && 4 * s + g < D) ? p.fc1_w[row * D + 4 * s + g] : 0.0f;
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int k = 16 * kb + 4 * g + r;
          a2[hb][kb][r] = (row < H && k < H) ? p.fc2_w[row * H + k] : 0.0f;
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int u = 16 * hb + 4 * g + r;
        bias1[hb][r] = u < H ? p.fc1_b[u] : 0.0f;
        bias2[hb][r] = u < H ? p.fc2_b[u] : 0.0f;
        w3[hb][r] = u < H ? p.fc3_w[u] : 0.0f;
      }
    }
    bias3 = p.fc3_b[0];
  }

  // xs: LDS tile [64 rows][kCriticIn], columns past the input width hold zeros
  __device__ __forceinline__ float forward(const float* xs, int lane) const {
    const int c = lane & 15, g = lane >> 4;
    float P[4];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      f32x4 h1[4][2], h2[4][2];
#pragma unroll
      for (int hb = 0; hb < 4; ++hb) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          h1[hb][b] = f32x4{bias1[hb][0], bias1[hb][1], bias1[hb][2], bias1[hb][3]};
          h2[hb][b] = f32x4{bias2[hb][0], bias2[hb][1], bias2[hb][2], bias2[hb][3]};
        }
      }
      float x[6][2];
#pragma unroll
      for (int s = 0; s < 6; ++s) {
#pragma unroll
        for (int b = 0; b < 2; ++b) x[s][b] = xs[(16 * (2 * half + b) + c) * kCriticIn + 4 * s + g];
      }
#pragma unroll
      for (int s = 0; s < 6; ++s) {
#pragma unroll
        for (int hb = 0; hb < 4; ++hb) {
#pragma unroll
          for (int b = 0; b < 2; ++b) h1[hb][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[hb][s], x[s][b], h1[hb][b], 0, 0, 0);
        }
      }
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float t0 = tanh_fast(h1[kb][0][r]), t1 = tanh_fast(h1[kb][1][r]);
#pragma unroll
          for (int ho = 0; ho < 4; ++ho) {
            h2[ho][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[ho][kb][r], t0, h2[ho][0], 0, 0, 0);
            h2[ho][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[ho][kb][r], t1, h2[ho][1], 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        float q[4];  // (four independent chains)
#pragma unroll
        for (int ho = 0; ho < 4; ++ho) {
          q[ho] = w3[ho][0] * tanh_fast(h2[ho][b][0]);
#pragma unroll
          for (int r = 1; r < 4; ++r) q[ho] = fmaf(w3[ho][r], tanh_fast(h2[ho][b][r]), q[ho]);
        }
        P[2 * half + b] = (q[0] + q[1]) + (q[2] + q[3]);
      }
    }
    // P[b] of lane (g, c) = row 16 b + c's sum over hidden group g.  The sum over g and the move of block b's result to lane
    // row g' = b: v_permlane16_swap exchanges the odd rows of one register with the even rows of another, v_permlane32_swap
    // the upper half with the lower half (ActorMfma::heads).
    const auto s01 = __builtin_amdgcn_permlane16_swap(__float_as_uint(P[0]), __float_as_uint(P[1]), false, false);
    const auto s23 = __builtin_amdgcn_permlane16_swap(__float_as_uint(P[2]), __float_as_uint(P[3]), false, false);
    const float q01 = __uint_as_float(s01[0]) + __uint_as_float(s01[1]);
    const float q23 = __uint_as_float(s23[0]) + __uint_as_float(s23[1]);
    const auto t = __builtin_amdgcn_permlane32_swap(__float_as_uint(q01), __float_as_uint(q23), false, false);
    return bias3 + (__uint_as_float(t[0]) + __uint_as_float(t[1]));
  }
};

// `nr` rows of width w, contiguous from `src`, into columns [col0, col0 + w) of the tile: linear (coalesced) dword loads, eight
// in flight per lane; the (row, column) of a lane's next element follows from 64 = q w + rem without a division per element.
__device__ __forceinline__ void critic_stage(float* xs, const float* src, int w, int col0, int nr, int lane) {
  if (w == 0) return;
  const int n = nr * w, q = 64 / w, rem = 64 - q * w;
  int r = lane / w, k = lane - r * w;
  for (int i0 = 0; i0 < n; i0 += 8 * 64) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = i0 + 64 * u + lane;
      v[u] = i < n ? src[i] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (i0 + 64 * u + lane < n) xs[r * kCriticIn + col0 + k] = v[u];
      r += q; k += rem;
      if (k >= w) { k -= w; ++r; }
    }
  }
}

// One wavefront per workgroup owns 64-row tiles and walks them grid-stride; the weights are loaded once per wave.
//   NEXT = false (qr_critic_values):       out[i stride] = V(row i).
//   NEXT = true  (qr_critic_next_values):  i = t N + n over [T][N]; out[i stride] = reset(i) ? V(final row i) : value[(i + N) stride].
//     A tile without a reset lane (wave ballot) only copies; otherwise the tile is evaluated and every lane SELECTS — the final
//     rows of envs that did not reset are meaningless (NaN included) and never reach an output: a row only feeds its own
//     MFMA column and its own lane's reduction.
template <bool NEXT>
__global__ __launch_bounds__(64) void critic_kernel(const CriticArgs a) {
  __shared__ float xs[64 * kCriticIn];
  const int lane = threadIdx.x;
  CriticMfma net;
  net.load(a, lane);
  for (int i = lane; i < 64 * kCriticIn; i += 64) xs[i] = 0.0f;  // the padding columns stay zero: staging never writes them
  __syncthreads();
  const int64_t tiles = (a.n_rows + 63) / 64;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t row0 = tile * 64, i = row0 + lane;
    const int nr = a.n_rows - row0 < 64 ? (int)(a.n_rows - row0) : 64;
    const bool active = lane < nr;
    bool reset = false;
    float carry = 0.0f;
    if (NEXT) {
      if (active) {
        for (int k = 0; k < a.n_agents; ++k) reset |= a.done[i * a.n_agents + k] != 0;
        if (a.truncated) reset |= a.truncated[i] != 0;
        carry = a.value[(i + a.n_envs) * a.stride];
      }
      if (__ballot(reset) == 0) {  // wave-uniform
        if (active) a.out[i * a.stride] = carry;
        continue;
      }
    }
    critic_stage(xs, a.rows0 + row0 * a.in0, a.in0, 0, nr, lane);
    critic_stage(xs, a.rows1 + row0 * a.in1, a.in1, a.in0, nr, lane);
    __syncthreads();
    const float v = net.forward(xs, lane);
    __syncthreads();  // the tile is read: the next one may be staged
    if (active) a.out[i * a.stride] = (!NEXT || reset) ? v : carry;
  }
}

}  // namespace qr
