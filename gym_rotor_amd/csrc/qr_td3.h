// qr_td3.h — part of the gfx950 quadrotor step library (included by quadrotor_kernels.hip, after qr_optim.h).
// The critic half of one TD3 minibatch update (TD3.train, algos/td3/td3.py:123-167, the non-CTDE branch) for the reference's twin
// critic MLP_Critic (algos/td3/td3_mlp.py:36-99; Q = fc3(relu(fc2(relu(fc1(sa))))), twice):
//   td3_target_kernel  (qr_twinq_target)   y = reward + discount (1 - done) min(Q1_targ, Q2_targ)(obs_next, a'), forward only
//   twinq_kernel + twinq_reduce_kernel (qr_twinq_grad)   mse(Q1, y) + mse(Q2, y) and its gradients for the twelve tensors
// The arrangement is ppo_critic_kernel's (qr_ppo_critic.h); this header carries its own copy, so that the PPO kernels' code does
// not depend on it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "quadrotor_hip.h"
#include "qr_actor.h"

namespace qr {

struct TwinQNetW { const float *fc1_w, *fc1_b, *fc2_w, *fc2_b, *fc3_w, *fc3_b; };  // one of the two Q networks

struct TwinQArgs {
  TwinQNetW net[2];                  // workgroup row blockIdx.y owns net[blockIdx.y]
  const float* obs;                  // [>= rows][obs_dim]
  const float* action;               // row i at action + i * act_stride (the column offset is already added)
  const float* y;                    // [B], by minibatch position
  const int64_t* index;              // [B] or NULL (rows 0..B-1)
  double* partials;                  // [2][grid][np]
  int64_t B, rows;
  int32_t obs_dim, action_dim, hidden, act_stride;
  float g_scale;                     // 2 / B: dLoss / dQ = g_scale * e
};

// Layout of one workgroup's partial vector = the order of one network's six gradient tensors (packed at the run-time sizes), then
// the two sums of `stats`: sum e^2, sum y.
struct TwinQLayout {
  int w1, b1, w2, b2, w3, b3, st, np;
  __host__ __device__ TwinQLayout(int D, int H)
      : w1(0), b1(H * D), w2(b1 + H), b2(w2 + H * H), w3(b2 + H), b3(w3 + H), st(b3 + 1), np(st + 2) {}
};

constexpr int kTqIn = 28;    // widest input row: obs_dim + action_dim (the Coupled critic has 23 + 4)
constexpr int kTqKS = 7;     // k-steps of layer 1
constexpr int kTqOnes = 28;  // the column of ones of the input tile: column 28 of the dW1 product is fc1_b's gradient
constexpr int kTqX = 33;     // row stride of the input tile: 28 inputs, the ones, zeros up to 32 columns (two 16-column blocks); odd
constexpr int kTqT = 65;     // row stride of the activation and delta tiles (64 units); odd

// The small vectors in LDS: fc1_b, fc2_b, fc3_w, each zero-padded to 64, then fc3_b.
constexpr int kTqB1 = 0, kTqB2 = 64, kTqW3 = 128, kTqB3 = 192, kTqVec = 196;
// fc1_w in LDS as layer 1's A operands in the lane map: entry (hb, s) of lane l at [(hb * kTqKS + s) * 64 + l].  Read per k-step
// and not kept resident: the seventh k-step of the 28-wide input would need 4 registers the gradient kernel does not have, and
// the 28 reads per half tile (conflict-free, one dword per lane) ride under 56 MFMAs.
constexpr int kTqW1 = 4 * kTqKS * 64;

__device__ __forceinline__ void twinq_fill_small(float* w1s, float* svec, const TwinQNetW& p, int D, int H, int lane) {
  const int c = lane & 15, g = lane >> 4;
#pragma unroll
  for (int hb = 0; hb < 4; ++hb) {
    const int row = 16 * hb + c;
#pragma unroll
    for (int s = 0; s < kTqKS; ++s) w1s[(hb * kTqKS + s) * 64 + lane] = (row < H && 4 * s + g < D) ? p.fc1_w[row * D + 4 * s + g] : 0.0f;
  }
  svec[kTqB1 + lane] = lane < H ? p.fc1_b[lane] : 0.0f;
  svec[kTqB2 + lane] = lane < H ? p.fc2_b[lane] : 0.0f;
  svec[kTqW3 + lane] = lane < H ? p.fc3_w[lane] : 0.0f;
  if (lane == 0) svec[kTqB3] = p.fc3_b[0];
}

// (An offset the compiler cannot see through keeps it from hoisting the loop-invariant LDS reads out of the tile loop into
//  registers these kernels do not have — ppo_critic_here's reason.)
__device__ __forceinline__ const float* twinq_here(const float* sm) {
  int z = 0;
  asm volatile("" : "+v"(z));
  return sm + z;
}

// Columns [col0, col0 + w) of the 64 rows src[r][0..w) into a tile of row stride `stride`: linear dword loads along each row,
// eight in flight per lane; a NULL row (past the batch) is zeros.
__device__ __forceinline__ void twinq_stage(float* xs, int stride, const float* const* src, int w, int col0, int lane) {
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
        xs[r * stride + col0 + k] = v[u];
      }
    }
  }
}

// Forward pass, deltas and the product W2^T dz2 in PpoCriticNet's lane map (qr_ppo_critic.h): units x rows, a lane holds unit
// 16 hb + 4 g + r of row 16 b + c in v[hb][b][r], two 16-row blocks (a half tile) at a time; fc2_w resident twice (a2 for the
// forward pass, a2t for W2^T dz2), fc1_w's operands read from LDS.  ReLU: the activation t = max(z, 0) is what is stored, and the
// delta through it is d * (t > 0).
struct TwinQNet {
  float a2[4][4][4], a2t[4][4][4];
  f32x4 acc1[4][2], acc2[4][4];
  float ab2[4][4], aw3[4][4], ab3;

  __device__ __forceinline__ void load(const TwinQNetW& p, int H, int lane) {
    const int c = lane & 15, g = lane >> 4;
#pragma unroll
    for (int hb = 0; hb < 4; ++hb) {
      const int row = 16 * hb + c;
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

// One wavefront per workgroup; workgroup row blockIdx.y owns ONE of the two networks and walks the minibatch's 64-row tiles
// grid-stride along x.  Per tile: gather the rows (index, clamped into [0, rows)) through the LDS tile — the observation row, then
// the action row — then per half tile: forward, the error against y, the deltas, and the three weight-gradient contractions into
// the resident accumulators.  At the end the workgroup writes ONE partial vector; twinq_reduce_kernel sums them.
__global__ __launch_bounds__(64) void twinq_kernel(const TwinQArgs a) {
  __shared__ float xs[64 * kTqX];          // the input tile; at the end: the lanes' VALU sums
  __shared__ float ts[32 * kTqT], ds[32 * kTqT];
  __shared__ float w1s[kTqW1], svec[kTqVec], ys[64];
  __shared__ const float* src0[64];
  __shared__ const float* src1[64];
  __shared__ double red64[64 * 2];
  const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
  const int D = a.obs_dim + a.action_dim, H = a.hidden;
  const TwinQNetW w = blockIdx.y ? a.net[1] : a.net[0];
  TwinQNet net;
  net.load(w, H, lane);
  twinq_fill_small(w1s, svec, w, D, H, lane);
  for (int i = lane; i < 64 * kTqX; i += 64) xs[i] = (i % kTqX == kTqOnes) ? 1.0f : 0.0f;  // staging writes columns < D only
  const float bias3 = w.fc3_b[0];
  double st[2] = {0.0, 0.0};
  __syncthreads();

  const int64_t tiles = (a.B + 63) / 64;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t row0 = tile * 64;
    {
      const bool active = row0 + lane < a.B;
      int64_t i = active ? (a.index ? a.index[row0 + lane] : row0 + lane) : 0;
      i = i < 0 ? 0 : (i >= a.rows ? a.rows - 1 : i);  // never a read outside the buffer
      src0[lane] = active ? a.obs + i * a.obs_dim : nullptr;
      src1[lane] = active ? a.action + i * a.act_stride : nullptr;
      ys[lane] = active ? a.y[row0 + lane] : 0.0f;
    }
    __syncthreads();
    twinq_stage(xs, kTqX, src0, a.obs_dim, 0, lane);
    twinq_stage(xs, kTqX, src1, a.action_dim, a.obs_dim, lane);
    __syncthreads();

#pragma unroll 1
    for (int half = 0; half < 2; ++half) {
      const float* sv = twinq_here(svec);
      const float* w1 = twinq_here(w1s);
      const float* xh = xs + 32 * half * kTqX;
      f32x4 h1[4][2], h2[4][2];
#pragma unroll
      for (int hb = 0; hb < 4; ++hb) {
        const int u = 16 * hb + 4 * g;
        h1[hb][0] = h1[hb][1] = f32x4{sv[kTqB1 + u], sv[kTqB1 + u + 1], sv[kTqB1 + u + 2], sv[kTqB1 + u + 3]};
        h2[hb][0] = h2[hb][1] = f32x4{sv[kTqB2 + u], sv[kTqB2 + u + 1], sv[kTqB2 + u + 2], sv[kTqB2 + u + 3]};
      }
#pragma unroll
      for (int s = 0; s < kTqKS; ++s) {
        float x[2];
#pragma unroll
        for (int b = 0; b < 2; ++b) x[b] = xh[(16 * b + c) * kTqX + 4 * s + g];
#pragma unroll
        for (int hb = 0; hb < 4; ++hb) {
          const float aw = w1[(hb * kTqKS + s) * 64 + lane];
#pragma unroll
          for (int b = 0; b < 2; ++b) h1[hb][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(aw, x[b], h1[hb][b], 0, 0, 0);
        }
      }
      // t1 = relu(z1): kept in registers for the (t1 > 0) mask, and into the activation tile for dW2
#pragma unroll
      for (int hb = 0; hb < 4; ++hb) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float t = fmaxf(h1[hb][b][r], 0.0f);
            h1[hb][b][r] = t;
            ts[(16 * b + c) * kTqT + 16 * hb + 4 * g + r] = t;
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
      // t2 = relu(z2); Q: the lane's dot over its 16 units, then the sum over the four 16-lane rows, which every one of them ends
      // with (a + b is commutative: the four lanes of a row hold the same bits)
      float gq[2];
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        float q[4];
#pragma unroll
        for (int ho = 0; ho < 4; ++ho) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float t = fmaxf(h2[ho][b][r], 0.0f);
            h2[ho][b][r] = t;
            q[ho] = r == 0 ? sv[kTqW3 + 16 * ho + 4 * g] * t : fmaf(sv[kTqW3 + 16 * ho + 4 * g + r], t, q[ho]);
          }
        }
        float P = (q[0] + q[1]) + (q[2] + q[3]);
        P += __shfl_xor(P, 16);
        P += __shfl_xor(P, 32);
        const int row = 32 * half + 16 * b + c;
        const bool active = row0 + row < a.B;
        const float y = ys[row], e = active ? (bias3 + P) - y : 0.0f;
        gq[b] = a.g_scale * e;  // dLoss / dQ of the row; 0 past the batch
        if (g == 0 && active) { st[0] += (double)e * (double)e; st[1] += (double)y; }
      }
      // fc3's gradients, and dz2 = g w3 (t2 > 0) over t2 in place
      net.ab3 += gq[0] + gq[1];
#pragma unroll
      for (int ho = 0; ho < 4; ++ho) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float w3 = sv[kTqW3 + 16 * ho + 4 * g + r];
          net.aw3[ho][r] += fmaf(gq[0], h2[ho][0][r], gq[1] * h2[ho][1][r]);
          float d[2];
#pragma unroll
          for (int b = 0; b < 2; ++b) {
            d[b] = h2[ho][b][r] > 0.0f ? gq[b] * w3 : 0.0f;
            h2[ho][b][r] = d[b];
            ds[(16 * b + c) * kTqT + 16 * ho + 4 * g + r] = d[b];
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
        for (int q = 0; q < 4; ++q) { A[q] = ds[(4 * s + g) * kTqT + 16 * q + c]; Bv[q] = ts[(4 * s + g) * kTqT + 16 * q + c]; }
#pragma unroll
        for (int ob = 0; ob < 4; ++ob) {
#pragma unroll
          for (int ib = 0; ib < 4; ++ib) net.acc2[ob][ib] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[ob], Bv[ib], net.acc2[ob][ib], 0, 0, 0);
        }
      }
      // dz1 = (W2^T dz2) (t1 > 0)
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
          for (int r = 0; r < 4; ++r) ds[(16 * b + c) * kTqT + 16 * hi + 4 * g + r] = h1[hi][b][r] > 0.0f ? d1[hi][b][r] : 0.0f;
        }
      }
      __syncthreads();
      // dW1 (and db1, the column of ones) += dz1^T x
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        float A[4], Bv[2];
#pragma unroll
        for (int q = 0; q < 4; ++q) A[q] = ds[(4 * s + g) * kTqT + 16 * q + c];
#pragma unroll
        for (int q = 0; q < 2; ++q) Bv[q] = xh[(4 * s + g) * kTqX + 16 * q + c];
#pragma unroll
        for (int ob = 0; ob < 4; ++ob) {
#pragma unroll
          for (int ib = 0; ib < 2; ++ib) net.acc1[ob][ib] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[ob], Bv[ib], net.acc1[ob][ib], 0, 0, 0);
        }
      }
      __syncthreads();  // both tiles are read: the next half (or the next rows) may be written
    }
  }

  const TwinQLayout Y(D, H);
  double* P = a.partials + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * Y.np;
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
        if (out < H && in == kTqOnes) P[Y.b1 + out] = (double)net.acc1[ob][ib][r];
      }
    }
  }
  // the per-lane sums: unit 16 ho + 4 g + r over its 16 lanes c, fc3_b over the 16 lanes of row g = 0, the statistics over the
  // lanes — each in lane order
#pragma unroll
  for (int ho = 0; ho < 4; ++ho) {
#pragma unroll
    for (int r = 0; r < 4; ++r) { xs[lane * kTqX + 4 * ho + r] = net.ab2[ho][r]; xs[lane * kTqX + 16 + 4 * ho + r] = net.aw3[ho][r]; }
  }
  xs[lane * kTqX + 32] = net.ab3;
  red64[lane * 2] = st[0];
  red64[lane * 2 + 1] = st[1];
  __syncthreads();
  if (lane < H) {
    const int ho = lane >> 4, gg = (lane >> 2) & 3, r = lane & 3;
    double s2 = 0.0, s3 = 0.0;
    for (int l = 0; l < 16; ++l) { s2 += (double)xs[(16 * gg + l) * kTqX + 4 * ho + r]; s3 += (double)xs[(16 * gg + l) * kTqX + 16 + 4 * ho + r]; }
    P[Y.b2 + lane] = s2;
    P[Y.w3 + lane] = s3;
  }
  if (lane < 2) {
    double s = 0.0;
    for (int l = 0; l < 64; ++l) s += red64[l * 2 + lane];
    P[Y.st + lane] = s;
  }
  if (lane == 63) {
    double s = 0.0;
    for (int l = 0; l < 16; ++l) s += (double)xs[l * kTqX + 32];
    P[Y.b3] = s;
  }
}

struct TwinQReduceArgs {
  const double* partials;   // [2][n_parts][np]
  float* grad[2][6];        // per network: fc1_w, fc1_b, fc2_w, fc2_b, fc3_w, fc3_b
  float* stats;             // [4]
  int32_t off[7];           // start of each gradient tensor in a partial vector; off[6] = the two sums
  int32_t n_parts, np;
  double B;
};

// Workgroup row blockIdx.y: one network.  Workgroups 0 .. gridDim.x - 2 of a row: sixteen consecutive gradient entries each — entry
// e of the result = the sum over the network's partial vectors of entry e, in float64 and in an order the grid alone fixes: sixteen
// slices of the partial vectors per entry, then a tree over the slices.  The last workgroup of row 0: the sums of both networks
// (256 strided slices each, then a tree), and from them `stats`.
__global__ __launch_bounds__(256) void twinq_reduce_kernel(const TwinQReduceArgs o) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  const int nn = blockIdx.y;
  if (blockIdx.x + 1 < gridDim.x) {
    const double* part = o.partials + (int64_t)nn * o.n_parts * o.np;
    const int q = t & 15, s = t >> 4, e = 16 * blockIdx.x + q;
    const bool valid = e < o.off[6];
    double sum = 0.0;
    if (valid)
      for (int p = s; p < o.n_parts; p += 16) sum += part[(int64_t)p * o.np + e];
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
      float* const* gr = nn ? o.grad[1] : o.grad[0];
      float* dst = gr[0];
#pragma unroll
      for (int j = 1; j < 6; ++j)
        if (k == j) dst = gr[j];
      dst[e - o.off[k]] = (float)red[t];
    }
    return;
  }
  if (nn) return;
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
  double sums[3];  // sum e1^2, sum y, sum e2^2
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const double* part = o.partials + (q == 2 ? (int64_t)o.n_parts * o.np : 0) + o.off[6] + (q == 1 ? 1 : 0);
    double mine = 0.0;
    for (int p = t; p < o.n_parts; p += 256) mine += part[(int64_t)p * o.np];
    sums[q] = tree(mine);
  }
  if (t == 0) {
    const double m1 = sums[0] / o.B, m2 = sums[2] / o.B;
    o.stats[0] = (float)(m1 + m2);
    o.stats[1] = (float)m1;
    o.stats[2] = (float)m2;
    o.stats[3] = (float)(sums[1] / o.B);
  }
}

// ------------------------------------------------------------------------------------------------------------------
// qr_twinq_target
// ------------------------------------------------------------------------------------------------------------------
struct Td3TargetArgs {
  ActorW actor;                      // pi_targ (AD > 0); log_std and the log_std head are NULL: never read
  TwinQNetW net[2];                  // Q1_targ, Q2_targ
  const float* obs_next;             // [>= rows][obs_dim]
  const float *reward, *done;        // element i at [i * rwd_stride] / [i * done_stride]
  const float* eps;                  // [B][action_dim] by minibatch position, or NULL
  const float* action_next;          // AD = 0: a' [B][action_dim] by minibatch position, used as it is
  const int64_t* index;
  float* y;                          // [B]
  int64_t B, rows;
  int32_t obs_dim, action_dim, hidden, rwd_stride, done_stride;
  float discount, target_noise, noise_clip, max_action;
};

// One target network, forward only: CriticMfma's arrangement (qr_critic.h) with ReLU, seven k-steps and fc1's operands and the small
// vectors in LDS; fc2_w resident.
struct TwinQFwd {
  float a2[4][4][4];

  __device__ __forceinline__ void load(const TwinQNetW& p, int H, int lane) {
    const int c = lane & 15, g = lane >> 4;
#pragma unroll
    for (int hb = 0; hb < 4; ++hb) {
      const int row = 16 * hb + c;
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int k = 16 * kb + 4 * g + r;
          a2[hb][kb][r] = (row < H && k < H) ? p.fc2_w[row * H + k] : 0.0f;
        }
      }
    }
  }

  // xs: the tile [64 rows][kTqX]; returns Q of row `lane`
  __device__ __forceinline__ float forward(const float* xs, const float* w1, const float* sv, int lane) const {
    const int c = lane & 15, g = lane >> 4;
    float P[4];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      f32x4 h1[4][2], h2[4][2];
#pragma unroll
      for (int hb = 0; hb < 4; ++hb) {
        const int u = 16 * hb + 4 * g;
        h1[hb][0] = h1[hb][1] = f32x4{sv[kTqB1 + u], sv[kTqB1 + u + 1], sv[kTqB1 + u + 2], sv[kTqB1 + u + 3]};
        h2[hb][0] = h2[hb][1] = f32x4{sv[kTqB2 + u], sv[kTqB2 + u + 1], sv[kTqB2 + u + 2], sv[kTqB2 + u + 3]};
      }
#pragma unroll
      for (int s = 0; s < kTqKS; ++s) {
        float x[2];
#pragma unroll
        for (int b = 0; b < 2; ++b) x[b] = xs[(16 * (2 * half + b) + c) * kTqX + 4 * s + g];
#pragma unroll
        for (int hb = 0; hb < 4; ++hb) {
          const float aw = w1[(hb * kTqKS + s) * 64 + lane];
#pragma unroll
          for (int b = 0; b < 2; ++b) h1[hb][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(aw, x[b], h1[hb][b], 0, 0, 0);
        }
      }
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float t0 = fmaxf(h1[kb][0][r], 0.0f), t1 = fmaxf(h1[kb][1][r], 0.0f);
#pragma unroll
          for (int ho = 0; ho < 4; ++ho) {
            h2[ho][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[ho][kb][r], t0, h2[ho][0], 0, 0, 0);
            h2[ho][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[ho][kb][r], t1, h2[ho][1], 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        float q[4];
#pragma unroll
        for (int ho = 0; ho < 4; ++ho) {
          q[ho] = sv[kTqW3 + 16 * ho + 4 * g] * fmaxf(h2[ho][b][0], 0.0f);
#pragma unroll
          for (int r = 1; r < 4; ++r) q[ho] = fmaf(sv[kTqW3 + 16 * ho + 4 * g + r], fmaxf(h2[ho][b][r], 0.0f), q[ho]);
        }
        P[2 * half + b] = (q[0] + q[1]) + (q[2] + q[3]);
      }
    }
    // P[b] of lane (g, c) = row 16 b + c's sum over hidden group g; the sum over g and the move of block b's result to lane row
    // g' = b (CriticMfma::forward)
    const auto s01 = __builtin_amdgcn_permlane16_swap(__float_as_uint(P[0]), __float_as_uint(P[1]), false, false);
    const auto s23 = __builtin_amdgcn_permlane16_swap(__float_as_uint(P[2]), __float_as_uint(P[3]), false, false);
    const float q01 = __uint_as_float(s01[0]) + __uint_as_float(s01[1]);
    const float q23 = __uint_as_float(s23[0]) + __uint_as_float(s23[1]);
    const auto t = __builtin_amdgcn_permlane32_swap(__float_as_uint(q01), __float_as_uint(q23), false, false);
    return sv[kTqB3] + (__uint_as_float(t[0]) + __uint_as_float(t[1]));
  }
};

// AD = the target actor's obs_dim: 23 or 15 (ActorMfma, hidden 16, 4 actions), 3 (ActorLds<3, 4, 1>), or 0: no actor, a' is
// supplied.  One wavefront per workgroup walks 64-row tiles grid-stride: gather obs_next rows (index, clamped) into the critic's
// input tile and the actor's tile, the actor's mean for the lane's own row, the smoothing noise and both clamps, a' into the
// columns behind the observation, then both target networks over the tile, min, and the Bellman line.  Lane l owns row l.
template <int AD>
__global__ __launch_bounds__(64) void td3_target_kernel(const Td3TargetArgs a) {
  constexpr int AA = AD == 3 ? 1 : 4;  // the actor's action_dim
  using Actor1 = ActorLds<3, 4, 1>;
  __shared__ float xs[64 * kTqX];
  __shared__ float as[AD > 0 ? 64 * AD : 4];
  __shared__ __attribute__((aligned(16))) float wsm[AD == 3 ? Actor1::SIZE : 4];
  __shared__ float w1s[2][kTqW1], svec[2][kTqVec];
  __shared__ const float* src0[64];
  const int lane = threadIdx.x;
  const int D = a.obs_dim + a.action_dim, H = a.hidden;
  TwinQFwd q1, q2;
  q1.load(a.net[0], H, lane);
  q2.load(a.net[1], H, lane);
  twinq_fill_small(w1s[0], svec[0], a.net[0], D, H, lane);
  twinq_fill_small(w1s[1], svec[1], a.net[1], D, H, lane);
  ActorMfma<(AD == 23 || AD == 15) ? AD : 23, false> actor;
  if constexpr (AD == 23 || AD == 15) actor.load(a.actor, lane);
  if constexpr (AD == 3) Actor1::fill(wsm, a.actor, lane);
  for (int i = lane; i < 64 * kTqX; i += 64) xs[i] = 0.0f;  // the padding columns stay zero: nothing below writes them
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
    twinq_stage(xs, kTqX, src0, a.obs_dim, 0, lane);
    if constexpr (AD > 0) twinq_stage(as, AD, src0, AD, 0, lane);
    __syncthreads();
    if constexpr (AD > 0) {
      float pre[AA], ls[AA];
      if constexpr (AD == 3) {
        float x[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) x[k] = as[lane * 3 + k];
        Actor1::heads(wsm, false, x, pre, ls);
      } else {
        actor.heads(as, lane, pre, ls);
      }
#pragma unroll
      for (int f = 0; f < AA; ++f) {
        float n = 0.0f;
        if (a.eps && active) n = fminf(fmaxf(a.target_noise * a.eps[j * AA + f], -a.noise_clip), a.noise_clip);
        xs[lane * kTqX + AD + f] = fminf(fmaxf(tanh_fast(pre[f]) + n, -a.max_action), a.max_action);
      }
    } else {
      for (int f = 0; f < a.action_dim; ++f) xs[lane * kTqX + a.obs_dim + f] = active ? a.action_next[j * a.action_dim + f] : 0.0f;
    }
    __syncthreads();
    const float v1 = q1.forward(xs, twinq_here(w1s[0]), twinq_here(svec[0]), lane);
    const float v2 = q2.forward(xs, twinq_here(w1s[1]), twinq_here(svec[1]), lane);
    __syncthreads();  // the tile is read: the next one may be staged
    if (active) a.y[j] = fmaf(a.discount * (1.0f - dn), fminf(v1, v2), rwd);
  }
}

}  // namespace qr
