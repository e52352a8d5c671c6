// qr_ppo_critic.h — part of the gfx950 quadrotor step library (included by quadrotor_kernels.hip, after qr_ppo.h).
// The critic half of one PPO minibatch update (PPO.train, algos/ppo/ppo.py:193-214): the mean squared error of MLP_Critic /
// MLP_Critic_CTDE against the TD target plus the L2 term on the three weight tensors, and the gradients with respect to the critic's
// six tensors, read from the rollout storage in place: ppo_critic_kernel + ppo_critic_reduce_kernel (qr_ppo_critic_grad).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "quadrotor_hip.h"
#include "qr_actor.h"
#include "qr_critic.h"

namespace qr {

struct PpoCriticArgs {
  const float *fc1_w, *fc1_b, *fc2_w, *fc2_b, *fc3_w, *fc3_b;
  const float *rows0, *rows1;        // [>= rows][in0], [>= rows][in1]: the observation rows (NULL where in0 / in1 is 0)
  const float* target;               // element i at target[i * tgt_stride]
  const int64_t* index;              // [B] or NULL (rows 0..B-1)
  double* partials;                  // [grid][np]
  int64_t B, rows;
  int32_t in0, in1, hidden, tgt_stride;
  float g_scale;                     // 2 / B: dLoss / dv = g_scale * e
};

// Layout of one workgroup's partial vector = the order of the six gradient tensors (packed at the run-time sizes), then the four
// sums of `stats`: sum e^2, sum e, sum y, sum y^2.
struct PpoCriticLayout {
  int w1, b1, w2, b2, w3, b3, st, np;
  __host__ __device__ PpoCriticLayout(int D, int H)
      : w1(0), b1(H * D), w2(b1 + H), b2(w2 + H * H), w3(b2 + H), b3(w3 + H), st(b3 + 1), np(st + 4) {}
};

constexpr int kPcOnes = kCriticIn;  // the column of ones of the input tile: column 24 of the dW1 product is fc1_b's gradient
constexpr int kPcX = 33;            // row stride of the input tile: 24 inputs, the ones, zeros up to 32 columns (two 16-column blocks); odd
constexpr int kPcT = 65;            // row stride of the activation and delta tiles (64 units); odd

// Forward pass, deltas and the product W2^T dz2 in CriticMfma's lane map (qr_critic.h; this kernel carries its own copy of the
// arrangement so that critic_kernel's code does not depend on it): units x rows, a lane holds unit 16 hb + 4 g + r of row
// 16 b + c in v[hb][b][r], two 16-row blocks (a half tile) at a time.
//   lane l: c = l & 15, g = l >> 4.   A: lane supplies A[c][k = g].  B: B[k = g][c].  D: lane holds D[4 g + r][c], r = 0..3.
//   z1 = W1 x, z2 = W2 t1:  as CriticMfma (weights resident as A operands; the lane's own t1 values are layer 2's B operands).
//   dz1^T = W2^T dz2^T:     the same trick backwards — the lane's own dz2[kb][b][r] is the B operand of k-step (kb, r),
//                           A = W2[16 kb + 4 g + r][16 hi + c], a second resident copy of fc2_w (transposed lane map).
// The WEIGHT GRADIENTS are contractions over rows, dW[out][in] = sum_rows delta[row][out] act[row][in], with k over the half
// tile's 32 rows (8 k-steps), as PpoNet::wgrad (qr_ppo.h): both operands need the row on lane >> 4, so the lanes write t1 and the
// deltas into two LDS tiles [32 rows][64 units] and read them back row-major:
//   A[c][k = g] = delta[row 4 s + g][16 ob + c],  B[k = g][c] = act[row 4 s + g][16 ib + c],  D: lane holds dW[16 ob + 4 g + r][16 ib + c].
// fc1_b's gradient is column 24 of the dW1 product (the input tile's column of ones); fc2_b's, fc3_w's and fc3_b's are per-lane
// VALU sums in the forward lane map, added over the lanes once at the end.  All accumulators stay in registers over a wave's tiles.
struct PpoCriticNet {
  float a1[4][6], a2[4][4][4], a2t[4][4][4];
  f32x4 acc1[4][2], acc2[4][4];
  float ab2[4][4], aw3[4][4], ab3;

  __device__ __forceinline__ void load(const PpoCriticArgs& p, int lane) {
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
          a2t[hb][kb][r] = (row < H && k < H) ? p.fc2_w[k * H + row] : 0.0f;
        }
      }
    }
#pragma unroll
    for (int ob = 0; ob < 4; ++ob) {
#pragma unroll
      for (int ib = 0; ib < 4; ++ib) acc2[ob][ib] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      acc1[ob][0] = acc1[ob][1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int r = 0; r < 4; ++r) ab2[ob][r] = aw3[ob][r] = 0.0f;
    }
    ab3 = 0.0f;
  }
};

// The small vectors in LDS: fc1_b, fc2_b, fc3_w, each zero-padded to 64.
constexpr int kPcB1 = 0, kPcB2 = 64, kPcW3 = 128, kPcVec = 192;

// (The small vectors are read from LDS where they are used: an offset the compiler cannot see through keeps it from hoisting the
//  loop-invariant reads out of the tile loop into registers this kernel does not have — PpoNet::here's reason.)
__device__ __forceinline__ const float* ppo_critic_here(const float* sm) {
  int z = 0;
  asm volatile("" : "+v"(z));
  return sm + z;
}

// Columns [col0, col0 + w) of the 64 rows src[r][0..w) into the input tile: linear dword loads along each row, eight in flight per
// lane; a NULL row (past the batch) is zeros.
__device__ __forceinline__ void ppo_critic_stage(float* xs, const float* const* src, int w, int col0, int lane) {
  const int n = 64 * w;
  for (int e0 = 0; e0 < n; e0 += 8 * 64) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int e = e0 + 64 * u + lane;
      v[u] = 0.0f;
      if (e < n) {
        const int r = e / w, k = e - r * w;
        const float* p = src[r];
        if (p) v[u] = p[k];
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int e = e0 + 64 * u + lane;
      if (e < n) {
        const int r = e / w, k = e - r * w;
        xs[r * kPcX + col0 + k] = v[u];
      }
    }
  }
}

// One wavefront per workgroup owns 64-row tiles of the minibatch and walks them grid-stride.  Per tile: gather the rows (index,
// clamped into [0, rows)) through the LDS tile — a CTDE row is formed there from its two sources — then per half tile: forward,
// the error against the target, the deltas, and the three weight-gradient contractions into the resident accumulators.  At the end
// the workgroup writes ONE partial vector; ppo_critic_reduce_kernel sums them.
__global__ __launch_bounds__(64) void ppo_critic_kernel(const PpoCriticArgs a) {
  __shared__ float xs[64 * kPcX];          // the input tile; at the end: the lanes' VALU sums
  __shared__ float ts[32 * kPcT], ds[32 * kPcT];
  __shared__ float svec[kPcVec], ys[64];
  __shared__ const float* src0[64];
  __shared__ const float* src1[64];
  __shared__ double red64[64 * 4];
  const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
  const int D = a.in0 + a.in1, H = a.hidden;
  PpoCriticNet net;
  net.load(a, lane);
  svec[kPcB1 + lane] = lane < H ? a.fc1_b[lane] : 0.0f;
  svec[kPcB2 + lane] = lane < H ? a.fc2_b[lane] : 0.0f;
  svec[kPcW3 + lane] = lane < H ? a.fc3_w[lane] : 0.0f;
  for (int i = lane; i < 64 * kPcX; i += 64) xs[i] = (i % kPcX == kPcOnes) ? 1.0f : 0.0f;  // staging writes columns < D only
  const float bias3 = a.fc3_b[0];
  double st[4] = {0.0, 0.0, 0.0, 0.0};
  __syncthreads();

  const int64_t tiles = (a.B + 63) / 64;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t row0 = tile * 64;
    {
      const bool active = row0 + lane < a.B;
      int64_t i = active ? (a.index ? a.index[row0 + lane] : row0 + lane) : 0;
      i = i < 0 ? 0 : (i >= a.rows ? a.rows - 1 : i);  // never a read outside the storage
      src0[lane] = active ? a.rows0 + i * a.in0 : nullptr;
      src1[lane] = active ? a.rows1 + i * a.in1 : nullptr;
      ys[lane] = active ? a.target[i * a.tgt_stride] : 0.0f;
    }
    __syncthreads();
    if (a.in0) ppo_critic_stage(xs, src0, a.in0, 0, lane);
    if (a.in1) ppo_critic_stage(xs, src1, a.in1, a.in0, lane);
    __syncthreads();

#pragma unroll 1
    for (int half = 0; half < 2; ++half) {
      const float* sv = ppo_critic_here(svec);
      const float* xh = xs + 32 * half * kPcX;
      f32x4 h1[4][2], h2[4][2];
#pragma unroll
      for (int hb = 0; hb < 4; ++hb) {
        const int u = 16 * hb + 4 * g;
        h1[hb][0] = h1[hb][1] = f32x4{sv[kPcB1 + u], sv[kPcB1 + u + 1], sv[kPcB1 + u + 2], sv[kPcB1 + u + 3]};
        h2[hb][0] = h2[hb][1] = f32x4{sv[kPcB2 + u], sv[kPcB2 + u + 1], sv[kPcB2 + u + 2], sv[kPcB2 + u + 3]};
      }
      {
        float x[6][2];
#pragma unroll
        for (int s = 0; s < 6; ++s) {
#pragma unroll
          for (int b = 0; b < 2; ++b) x[s][b] = xh[(16 * b + c) * kPcX + 4 * s + g];
        }
#pragma unroll
        for (int s = 0; s < 6; ++s) {
#pragma unroll
          for (int hb = 0; hb < 4; ++hb) {
#pragma unroll
            for (int b = 0; b < 2; ++b) h1[hb][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(net.a1[hb][s], x[s][b], h1[hb][b], 0, 0, 0);
          }
        }
      }
      // t1 = tanh(z1): kept in registers for (1 - t1^2), and into the activation tile for dW2
#pragma unroll
      for (int hb = 0; hb < 4; ++hb) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float t = tanh_fast(h1[hb][b][r]);
            h1[hb][b][r] = t;
            ts[(16 * b + c) * kPcT + 16 * hb + 4 * g + r] = t;
          }
        }
      }
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
          for (int ho = 0; ho < 4; ++ho) {
#pragma unroll
            for (int b = 0; b < 2; ++b) h2[ho][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(net.a2[ho][kb][r], h1[kb][b][r], h2[ho][b], 0, 0, 0);
          }
        }
      }
      // t2 = tanh(z2); the value: the lane's dot over its 16 units, then the sum over the four 16-lane rows, which every one of
      // them ends with (a + b is commutative: the four lanes of a row hold the same bits)
      float gq[2];
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        float q[4];
#pragma unroll
        for (int ho = 0; ho < 4; ++ho) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float t = tanh_fast(h2[ho][b][r]);
            h2[ho][b][r] = t;
            q[ho] = r == 0 ? sv[kPcW3 + 16 * ho + 4 * g] * t : fmaf(sv[kPcW3 + 16 * ho + 4 * g + r], t, q[ho]);
          }
        }
        float P = (q[0] + q[1]) + (q[2] + q[3]);
        P += __shfl_xor(P, 16);
        P += __shfl_xor(P, 32);
        const int row = 32 * half + 16 * b + c;
        const bool active = row0 + row < a.B;
        const float y = ys[row], e = active ? (bias3 + P) - y : 0.0f;
        gq[b] = a.g_scale * e;  // dLoss / dv of the row; 0 past the batch
        if (g == 0 && active) {
          st[0] += (double)e * (double)e; st[1] += (double)e; st[2] += (double)y; st[3] += (double)y * (double)y;
        }
      }
      // fc3's gradients, and dz2 = g w3 (1 - t2^2) over t2 in place
      net.ab3 += gq[0] + gq[1];
#pragma unroll
      for (int ho = 0; ho < 4; ++ho) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float w = sv[kPcW3 + 16 * ho + 4 * g + r];
          net.aw3[ho][r] += fmaf(gq[0], h2[ho][0][r], gq[1] * h2[ho][1][r]);
          float d[2];
#pragma unroll
          for (int b = 0; b < 2; ++b) {
            d[b] = gq[b] * w * fmaf(-h2[ho][b][r], h2[ho][b][r], 1.0f);
            h2[ho][b][r] = d[b];
            ds[(16 * b + c) * kPcT + 16 * ho + 4 * g + r] = d[b];
          }
          net.ab2[ho][r] += d[0] + d[1];
        }
      }
      __syncthreads();
      // dW2 += dz2^T t1 over the half tile's rows
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        float A[4], Bv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { A[q] = ds[(4 * s + g) * kPcT + 16 * q + c]; Bv[q] = ts[(4 * s + g) * kPcT + 16 * q + c]; }
#pragma unroll
        for (int ob = 0; ob < 4; ++ob) {
#pragma unroll
          for (int ib = 0; ib < 4; ++ib) net.acc2[ob][ib] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[ob], Bv[ib], net.acc2[ob][ib], 0, 0, 0);
        }
      }
      // dz1 = (W2^T dz2) (1 - t1^2)
      f32x4 d1[4][2];
#pragma unroll
      for (int hi = 0; hi < 4; ++hi) d1[hi][0] = d1[hi][1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
          for (int hi = 0; hi < 4; ++hi) {
#pragma unroll
            for (int b = 0; b < 2; ++b) d1[hi][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(net.a2t[hi][kb][r], h2[kb][b][r], d1[hi][b], 0, 0, 0);
          }
        }
      }
      __syncthreads();  // the delta tile is read: dz1 takes its place
#pragma unroll
      for (int hi = 0; hi < 4; ++hi) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
#pragma unroll
          for (int r = 0; r < 4; ++r) ds[(16 * b + c) * kPcT + 16 * hi + 4 * g + r] = d1[hi][b][r] * fmaf(-h1[hi][b][r], h1[hi][b][r], 1.0f);
        }
      }
      __syncthreads();
      // dW1 (and db1, the column of ones) += dz1^T x
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        float A[4], Bv[2];
#pragma unroll
        for (int q = 0; q < 4; ++q) A[q] = ds[(4 * s + g) * kPcT + 16 * q + c];
#pragma unroll
        for (int q = 0; q < 2; ++q) Bv[q] = xh[(4 * s + g) * kPcX + 16 * q + c];
#pragma unroll
        for (int ob = 0; ob < 4; ++ob) {
#pragma unroll
          for (int ib = 0; ib < 2; ++ib) net.acc1[ob][ib] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[ob], Bv[ib], net.acc1[ob][ib], 0, 0, 0);
        }
      }
      __syncthreads();  // both tiles are read: the next half (or the next rows) may be written
    }
  }

  const PpoCriticLayout Y(D, H);
  double* P = a.partials + (int64_t)blockIdx.x * Y.np;
#pragma unroll
  for (int ob = 0; ob < 4; ++ob) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int out = 16 * ob + 4 * g + r;
#pragma unroll
      for (int ib = 0; ib < 4; ++ib) {
        const int in = 16 * ib + c;
        if (out < H && in < H) P[Y.w2 + out * H + in] = (double)net.acc2[ob][ib][r];
      }
#pragma unroll
      for (int ib = 0; ib < 2; ++ib) {
        const int in = 16 * ib + c;
        if (out < H && in < D) P[Y.w1 + out * D + in] = (double)net.acc1[ob][ib][r];
        if (out < H && in == kPcOnes) P[Y.b1 + out] = (double)net.acc1[ob][ib][r];
      }
    }
  }
  // the per-lane sums: unit 16 ho + 4 g + r over its 16 lanes c, fc3_b over the 16 lanes of row g = 0, the statistics over the
  // lanes — each in lane order
#pragma unroll
  for (int ho = 0; ho < 4; ++ho) {
#pragma unroll
    for (int r = 0; r < 4; ++r) { xs[lane * kPcX + 4 * ho + r] = net.ab2[ho][r]; xs[lane * kPcX + 16 + 4 * ho + r] = net.aw3[ho][r]; }
  }
  xs[lane * kPcX + 32] = net.ab3;
#pragma unroll
  for (int q = 0; q < 4; ++q) red64[lane * 4 + q] = st[q];
  __syncthreads();
  if (lane < H) {
    const int ho = lane >> 4, gg = (lane >> 2) & 3, r = lane & 3;
    double s2 = 0.0, s3 = 0.0;
    for (int l = 0; l < 16; ++l) { s2 += (double)xs[(16 * gg + l) * kPcX + 4 * ho + r]; s3 += (double)xs[(16 * gg + l) * kPcX + 16 + 4 * ho + r]; }
    P[Y.b2 + lane] = s2;
    P[Y.w3 + lane] = s3;
  }
  if (lane < 4) {
    double s = 0.0;
    for (int l = 0; l < 64; ++l) s += red64[l * 4 + lane];
    P[Y.st + lane] = s;
  }
  if (lane == 63) {
    double s = 0.0;
    for (int l = 0; l < 16; ++l) s += (double)xs[l * kPcX + 32];
    P[Y.b3] = s;
  }
}

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

// Workgroups 0 .. gridDim.x - 2: sixteen consecutive gradient entries each — entry e of the result = the sum over the partial
// vectors of entry e, in float64 and in an order the grid alone fixes: sixteen slices of the partial vectors per entry, then a
// tree over the slices — plus 2 l2_reg W on the weight tensors.  The last workgroup: the four sums and the three ||W||^2 (256
// strided slices each, then a tree), and from them `stats`.
__global__ __launch_bounds__(256) void ppo_critic_reduce_kernel(const PpoCriticReduceArgs o) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  if (blockIdx.x + 1 < gridDim.x) {
    const int q = t & 15, s = t >> 4, e = 16 * blockIdx.x + q;
    const bool valid = e < o.off[6];
    double sum = 0.0;
    if (valid)
      for (int p = s; p < o.n_parts; p += 16) sum += o.partials[(int64_t)p * o.np + e];
    red[t] = sum;
    __syncthreads();
    for (int w = 8; w >= 1; w >>= 1) {
      if (s < w) red[t] += red[t + 16 * w];
      __syncthreads();
    }
    if (s == 0 && valid) {
      int k = 0;
#pragma unroll
      for (int j = 1; j < 6; ++j)
        if (e >= o.off[j]) k = j;
      double v = red[t];
      if ((k & 1) == 0) v += 2.0 * (double)o.l2_reg * (double)o.weight[k >> 1][e - o.off[k]];
      o.grad[k][e - o.off[k]] = (float)v;
    }
    return;
  }
  auto tree = [&](double mine) {
    __syncthreads();
    red[t] = mine;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
      if (t < w) red[t] += red[t + w];
      __syncthreads();
    }
    return red[0];
  };
  double sums[4], norm = 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    double mine = 0.0;
    for (int p = t; p < o.n_parts; p += 256) mine += o.partials[(int64_t)p * o.np + o.off[6] + q];
    sums[q] = tree(mine);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int n = o.off[2 * k + 1] - o.off[2 * k];
    double mine = 0.0;
    for (int j = t; j < n; j += 256) { const double w = (double)o.weight[k][j]; mine += w * w; }
    norm += tree(mine);
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
