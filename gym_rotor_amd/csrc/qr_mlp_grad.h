// qr_mlp_grad.h — part of the gfx950 quadrotor step library (included by qr_ppo_critic.h and qr_td3.h only).
// What the update-side kernels of a three-layer MLP critic v = fc3(act(fc2(act(fc1(x))))) share: one half tile (32 rows) forwards
// and backwards into resident gradient accumulators (mlp_grad_half), the partial vector a workgroup leaves behind
// (MlpGradLayout, mlp_grad_write), the staging of gathered rows, the tile walk around them (mlp_grad_walk) and the sums of the reduce
// kernels.  A kernel supplies a traits type (activation, input width, where layer 1's A operands live) and a rule (rows, targets, statistics).
// Nothing a rollout, step, evaluate, actor or critic_kernel instantiation compiles includes this file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "qr_actor.h"

namespace qr {

struct MlpNetW { const float *fc1_w, *fc1_b, *fc2_w, *fc2_b, *fc3_w, *fc3_b; };  // one network

// Layout of one workgroup's partial vector = the order of the six gradient tensors (packed at the run-time sizes), then the
// kernel's n_sums statistics.
struct MlpGradLayout {
  int w1, b1, w2, b2, w3, b3, st, np;
  __host__ __device__ MlpGradLayout(int D, int H, int n_sums)
      : w1(0), b1(H * D), w2(b1 + H), b2(w2 + H * H), w3(b2 + H), b3(w3 + H), st(b3 + 1), np(st + n_sums) {}
  // start of each gradient tensor in a partial vector; off[6] = the statistics
  __host__ void starts(int32_t (&off)[7]) const {
    const int s[7] = {w1, b1, w2, b2, w3, b3, st};
    for (int k = 0; k < 7; ++k) off[k] = s[k];
  }
};

constexpr int kMgX = 33;  // row stride of the input tile: the inputs, the column of ones, zeros up to 32 columns (two 16-column blocks); odd
constexpr int kMgT = 65;  // row stride of the activation and delta tiles (64 units); odd
// The small vectors in LDS: fc1_b, fc2_b, fc3_w, each zero-padded to 64 (then, where a kernel wants it there, fc3_b).
constexpr int kMgB1 = 0, kMgB2 = 64, kMgW3 = 128, kMgB3 = 192;

__device__ __forceinline__ void fill_vecs(float* svec, const MlpNetW& p, int H, int lane) {
  svec[kMgB1 + lane] = lane < H ? p.fc1_b[lane] : 0.0f;
  svec[kMgB2 + lane] = lane < H ? p.fc2_b[lane] : 0.0f;
  svec[kMgW3 + lane] = lane < H ? p.fc3_w[lane] : 0.0f;
}

// An offset the compiler cannot see through: LDS reads behind it stay where they are written instead of being hoisted out of
// the tile loop into registers these kernels do not have (PpoNet::here's reason, qr_ppo.h).
__device__ __forceinline__ const float* lds_here(const float* sm) {
  int z = 0;
  asm volatile("" : "+v"(z));
  return sm + z;
}

// Columns [col0, col0 + w) of the 64 rows src[r][0..w) into a tile of row stride `stride`: linear dword loads along each row,
// eight in flight per lane; a NULL row (past the batch) is zeros.
__device__ __forceinline__ void stage_rows(float* xs, int stride, const float* const* src, int w, int col0, int lane) {
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

// fc2_w as resident A operands in CriticMfma's lane map (qr_critic.h): a2[hb][kb][r] = W2[16 hb + c][16 kb + 4 g + r] for the
// forward pass, and (the second form) a2t = the same of W2^T for the product W2^T dz2; zero past H.
__device__ __forceinline__ void load_fc2(float (&a2)[4][4][4], const float* fc2_w, int H, int lane) {
  const int c = lane & 15, g = lane >> 4;
#pragma unroll
  for (int hb = 0; hb < 4; ++hb) {
    const int row = 16 * hb + c;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k = 16 * kb + 4 * g + r;
        a2[hb][kb][r] = (row < H && k < H) ? fc2_w[row * H + k] : 0.0f;
      }
    }
  }
}

__device__ __forceinline__ void load_fc2(float (&a2)[4][4][4], float (&a2t)[4][4][4], const float* fc2_w, int H, int lane) {
  const int c = lane & 15, g = lane >> 4;
#pragma unroll
  for (int hb = 0; hb < 4; ++hb) {
    const int row = 16 * hb + c;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k = 16 * kb + 4 * g + r;
        a2[hb][kb][r] = (row < H && k < H) ? fc2_w[row * H + k] : 0.0f;
        a2t[hb][kb][r] = (row < H && k < H) ? fc2_w[k * H + row] : 0.0f;
      }
    }
  }
}

// The gradient accumulators, resident over all tiles of a wave: dW1 (with db1 in the column of ones) and dW2 as MFMA blocks,
// db2, dW3 and db3 as per-lane VALU sums in the forward lane map.
struct MlpGradAcc {
  f32x4 acc1[4][2], acc2[4][4];
  float ab2[4][4], aw3[4][4], ab3;

  __device__ __forceinline__ void zero() {
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

// The forward pieces of mlp_grad_half (below; its lane map), for one half tile (h[hb][b][r]: unit 16 hb + 4 g + r of row 16 b + c).
// h1 = fc1_b, h2 = fc2_b on every row
__device__ __forceinline__ void mlp_bias(f32x4 (&h1)[4][2], f32x4 (&h2)[4][2], const float* sv, int lane) {
  const int g = lane >> 4;
#pragma unroll
  for (int hb = 0; hb < 4; ++hb) {
    const int u = 16 * hb + 4 * g;
    h1[hb][0] = h1[hb][1] = f32x4{sv[kMgB1 + u], sv[kMgB1 + u + 1], sv[kMgB1 + u + 2], sv[kMgB1 + u + 3]};
    h2[hb][0] = h2[hb][1] = f32x4{sv[kMgB2 + u], sv[kMgB2 + u + 1], sv[kMgB2 + u + 2], sv[kMgB2 + u + 3]};
  }
}

// h1 += W1 x over the half's 32 input rows xh (stride kMgX); MFMA order (s, hb, b)
template <class L>
__device__ __forceinline__ void mlp_layer1(f32x4 (&h1)[4][2], const L& l1, const float* xh, int lane) {
  const int c = lane & 15, g = lane >> 4;
  const float* xl = xh + c * kMgX + g;  // the lane's B operand of (s, b): x[row 16 b + c][4 s + g]
  float x[L::KS][2];
#pragma unroll
  for (int s = 0; s < L::KS; ++s) {
#pragma unroll
    for (int b = 0; b < 2; ++b) x[s][b] = xl[16 * b * kMgX + 4 * s];
  }
#pragma unroll
  for (int s = 0; s < L::KS; ++s) {
#pragma unroll
    for (int hb = 0; hb < 4; ++hb) {
      const float aw = l1.a1(hb, s, lane);
#pragma unroll
      for (int b = 0; b < 2; ++b) h1[hb][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(aw, x[s][b], h1[hb][b], 0, 0, 0);
    }
  }
}

// h2 += W2 t1, the lane's own t1 values as B operands; MFMA order (kb, r, ho, b)
__device__ __forceinline__ void mlp_layer2(f32x4 (&h2)[4][2], const float (&a2)[4][4][4], const f32x4 (&t1)[4][2]) {
#pragma unroll
  for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int ho = 0; ho < 4; ++ho) {
#pragma unroll
        for (int b = 0; b < 2; ++b) h2[ho][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[ho][kb][r], t1[kb][b][r], h2[ho][b], 0, 0, 0);
      }
    }
  }
}

// One half tile forwards and backwards, in CriticMfma's lane map (qr_critic.h): units x rows, a lane holds unit 16 hb + 4 g + r of
// row 16 b + c in v[hb][b][r], two 16-row blocks at a time.
//   lane l: c = l & 15, g = l >> 4.   A: lane supplies A[c][k = g].  B: B[k = g][c].  D: lane holds D[4 g + r][c], r = 0..3.
//   z1 = W1 x, z2 = W2 t1:  as CriticMfma (weights as A operands; the lane's own t1 values are layer 2's B operands).
//   dz1^T = W2^T dz2^T:     the same trick backwards — the lane's own dz2[kb][b][r] is the B operand of k-step (kb, r),
//                           A = W2[16 kb + 4 g + r][16 hi + c], the second resident copy of fc2_w (a2t).
// The WEIGHT GRADIENTS are contractions over rows, dW[out][in] = sum_rows delta[row][out] act[row][in], with k over the half
// tile's 32 rows (8 k-steps), as PpoNet::wgrad (qr_ppo.h): both operands need the row on lane >> 4, so the lanes write t1 and the
// deltas into two LDS tiles [32 rows][64 units] (ts, ds) and read them back row-major:
//   A[c][k = g] = delta[row 4 s + g][16 ob + c],  B[k = g][c] = act[row 4 s + g][16 ib + c],  D: lane holds dW[16 ob + 4 g + r][16 ib + c].
// fc1_b's gradient is column L::ONES of the dW1 product (the input tile's column of ones); fc2_b's, fc3_w's and fc3_b's are per-lane
// VALU sums, added over the lanes once at the end (mlp_grad_write).
// The traits L: act(z), dact(t, d) = d act'(z) written in t = act(z); KS k-steps of layer 1 (inputs <= 4 KS), ONES; and
// a1(hb, s, lane), layer 1's A operand W1[16 hb + c][4 s + g] — from a resident array or from LDS.
// xh: the half's 32 input rows (stride kMgX); sv: the small vectors (behind lds_here); ys: the half's 32 targets; n_active: how
// many of the half's rows are inside the batch; stat(e, y): called once per active row (on the lanes g = 0).
template <class L, class Stat>
__device__ __forceinline__ void mlp_grad_half(MlpGradAcc& acc, const L& l1, const float (&a2)[4][4][4], const float (&a2t)[4][4][4],
                                              const float* sv, const float* xs, float* ts, float* ds, const float* ys, int half, int64_t row0, int64_t B,
                                              float bias3, float g_scale, int lane, Stat&& stat) {
  const int c = lane & 15, g = lane >> 4;
  const float* xh = xs + 32 * half * kMgX;
  f32x4 h1[4][2], h2[4][2];
  mlp_bias(h1, h2, sv, lane);
  mlp_layer1(h1, l1, xh, lane);
  // t1 = act(z1): kept in registers for act', and into the activation tile for dW2
#pragma unroll
  for (int hb = 0; hb < 4; ++hb) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float t = L::act(h1[hb][b][r]);
        h1[hb][b][r] = t;
        ts[(16 * b + c) * kMgT + 16 * hb + 4 * g + r] = t;
      }
    }
  }
  mlp_layer2(h2, a2, h1);
  // t2 = act(z2); the value: the lane's dot over its 16 units, then the sum over the four 16-lane rows, which every one of
  // them ends with (a + b is commutative: the four lanes of a row hold the same bits)
  float gq[2];
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const float* sq = lds_here(sv);  // fc3_w behind an offset of its own per use: or its sixteen values stay in registers from here on
    float q[4];
#pragma unroll
    for (int ho = 0; ho < 4; ++ho) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float t = L::act(h2[ho][b][r]);
        h2[ho][b][r] = t;
        q[ho] = r == 0 ? sq[kMgW3 + 16 * ho + 4 * g] * t : fmaf(sq[kMgW3 + 16 * ho + 4 * g + r], t, q[ho]);
      }
    }
    float P = (q[0] + q[1]) + (q[2] + q[3]);
    P += __shfl_xor(P, 16);
    P += __shfl_xor(P, 32);
    const int row = 32 * half + 16 * b + c;
    const bool active = row0 + row < B;
    const float y = ys[row], e = active ? (bias3 + P) - y : 0.0f;
    gq[b] = g_scale * e;  // dLoss / dv of the row; 0 past the batch
    if (g == 0 && active) stat(e, y);
  }
  // fc3's gradients, and dz2 = g w3 act'(z2) over t2 in place
  const float* sw = lds_here(sv);
  acc.ab3 += gq[0] + gq[1];
#pragma unroll
  for (int ho = 0; ho < 4; ++ho) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float w = sw[kMgW3 + 16 * ho + 4 * g + r];
      acc.aw3[ho][r] += fmaf(gq[0], h2[ho][0][r], gq[1] * h2[ho][1][r]);
      float d[2];
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        d[b] = L::dact(h2[ho][b][r], gq[b] * w);
        h2[ho][b][r] = d[b];
        ds[(16 * b + c) * kMgT + 16 * ho + 4 * g + r] = d[b];
      }
      acc.ab2[ho][r] += d[0] + d[1];
    }
  }
  __syncthreads();
  // dW2 += dz2^T t1 over the half tile's rows
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    float A[4], Bv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { A[q] = ds[(4 * s + g) * kMgT + 16 * q + c]; Bv[q] = ts[(4 * s + g) * kMgT + 16 * q + c]; }
#pragma unroll
    for (int ob = 0; ob < 4; ++ob) {
#pragma unroll
      for (int ib = 0; ib < 4; ++ib) acc.acc2[ob][ib] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[ob], Bv[ib], acc.acc2[ob][ib], 0, 0, 0);
    }
  }
  // dz1 = (W2^T dz2) act'(z1)
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
        for (int b = 0; b < 2; ++b) d1[hi][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2t[hi][kb][r], h2[kb][b][r], d1[hi][b], 0, 0, 0);
      }
    }
  }
  __syncthreads();  // the delta tile is read: dz1 takes its place
#pragma unroll
  for (int hi = 0; hi < 4; ++hi) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
#pragma unroll
      for (int r = 0; r < 4; ++r) ds[(16 * b + c) * kMgT + 16 * hi + 4 * g + r] = L::dact(h1[hi][b][r], d1[hi][b][r]);
    }
  }
  __syncthreads();
  // dW1 (and db1, the column of ones) += dz1^T x
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    float A[4], Bv[2];
#pragma unroll
    for (int q = 0; q < 4; ++q) A[q] = ds[(4 * s + g) * kMgT + 16 * q + c];
#pragma unroll
    for (int q = 0; q < 2; ++q) Bv[q] = xh[(4 * s + g) * kMgX + 16 * q + c];
#pragma unroll
    for (int ob = 0; ob < 4; ++ob) {
#pragma unroll
      for (int ib = 0; ib < 2; ++ib) acc.acc1[ob][ib] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[ob], Bv[ib], acc.acc1[ob][ib], 0, 0, 0);
    }
  }
  __syncthreads();  // both tiles are read: the next half (or the next rows) may be written
}

// The workgroup's ONE partial vector: dW1, db1 (column `ones` of the dW1 product), dW2 from the MFMA accumulators, then the
// per-lane sums through LDS (xs: the input tile, free by now; red64: [64][NS] doubles) — unit 16 ho + 4 g + r of db2 and dW3 over
// its 16 lanes c, db3 over the 16 lanes of row g = 0, the NS statistics over the 64 lanes — each in lane order.
template <int NS>
__device__ __forceinline__ void mlp_grad_write(double* P, const MlpGradLayout& Y, const MlpGradAcc& acc, const double (&st)[NS], float* xs,
                                               double* red64, int ones, int D, int H, int lane) {
  const int c = lane & 15, g = lane >> 4;
#pragma unroll
  for (int ob = 0; ob < 4; ++ob) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int out = 16 * ob + 4 * g + r;
#pragma unroll
      for (int ib = 0; ib < 4; ++ib) {
        const int in = 16 * ib + c;
        if (out < H && in < H) P[Y.w2 + out * H + in] = (double)acc.acc2[ob][ib][r];
      }
#pragma unroll
      for (int ib = 0; ib < 2; ++ib) {
        const int in = 16 * ib + c;
        if (out < H && in < D) P[Y.w1 + out * D + in] = (double)acc.acc1[ob][ib][r];
        if (out < H && in == ones) P[Y.b1 + out] = (double)acc.acc1[ob][ib][r];
      }
    }
  }
#pragma unroll
  for (int ho = 0; ho < 4; ++ho) {
#pragma unroll
    for (int r = 0; r < 4; ++r) { xs[lane * kMgX + 4 * ho + r] = acc.ab2[ho][r]; xs[lane * kMgX + 16 + 4 * ho + r] = acc.aw3[ho][r]; }
  }
  xs[lane * kMgX + 32] = acc.ab3;
#pragma unroll
  for (int q = 0; q < NS; ++q) red64[lane * NS + q] = st[q];
  __syncthreads();
  if (lane < H) {
    const int ho = lane >> 4, gg = (lane >> 2) & 3, r = lane & 3;
    double s2 = 0.0, s3 = 0.0;
    for (int l = 0; l < 16; ++l) { s2 += (double)xs[(16 * gg + l) * kMgX + 4 * ho + r]; s3 += (double)xs[(16 * gg + l) * kMgX + 16 + 4 * ho + r]; }
    P[Y.b2 + lane] = s2;
    P[Y.w3 + lane] = s3;
  }
  if (lane < NS) {
    double s = 0.0;
    for (int l = 0; l < 64; ++l) s += red64[l * NS + lane];
    P[Y.st + lane] = s;
  }
  if (lane == 63) {
    double s = 0.0;
    for (int l = 0; l < 16; ++l) s += (double)xs[l * kMgX + 32];
    P[Y.b3] = s;
  }
}

// What ppo_critic_kernel (qr_ppo_critic.h) and twinq_kernel (qr_td3.h) share: the tile walk.  One wavefront per workgroup; workgroup
// row blockIdx.y owns ONE network and walks the minibatch's 64-row tiles grid-stride along x.  Per tile: gather the rows (index,
// clamped into [0, rows)) through the LDS tile — each row is formed there from its SRC sources — then per half tile mlp_grad_half
// into the resident accumulators.  At the end the workgroup writes ONE partial vector, [blockIdx.y][blockIdx.x].
// A Rule supplies what is the algorithm's own: Args (B, rows, index, hidden, g_scale and partials carry the same names in both), the
// traits L1, SUMS statistics, the sizes W1S / SVEC of the LDS arrays behind layer 1's operands and the small vectors, SRC (how many
// sources a row has: two, or the four of a centralized critic, qr_td3.h), SKIP_EMPTY (a source of width 0 is not staged), and
//   width(a, s), net(a)              the width of source s; the network of this workgroup row
//   fill(w1s, svec, w, D, H, lane)   layer 1's operands and the small vectors, once per workgroup
//   layer1(w1s)                      layer 1's operands as mlp_grad_half takes them, once per half tile
//   row(a, i, s)                     source s of storage row i
//   target(a, i, j), stat(st, e, y)  the target of storage row i at minibatch position j; the statistics of one active row
template <class Rule>
__device__ __forceinline__ void mlp_grad_walk(const typename Rule::Args& a) {
  using L1 = typename Rule::L1;
  __shared__ float xs[64 * kMgX];          // the input tile; at the end: the lanes' VALU sums
  __shared__ float ts[32 * kMgT], ds[32 * kMgT];
  __shared__ float w1s[Rule::W1S], svec[Rule::SVEC], ys[64];
  __shared__ const float* src[Rule::SRC][64];
  __shared__ double red64[64 * Rule::SUMS];
  const int lane = threadIdx.x;
  int in[Rule::SRC], D = 0;
#pragma unroll
  for (int s = 0; s < Rule::SRC; ++s) { in[s] = Rule::width(a, s); D += in[s]; }
  const int H = a.hidden;
  const MlpNetW w = Rule::net(a);
  Rule rule;
  float a2[4][4][4], a2t[4][4][4];
  MlpGradAcc acc;
  load_fc2(a2, a2t, w.fc2_w, H, lane);
  acc.zero();
  rule.fill(w1s, svec, w, D, H, lane);
  for (int i = lane; i < 64 * kMgX; i += 64) xs[i] = (i % kMgX == L1::ONES) ? 1.0f : 0.0f;  // staging writes columns < D only
  const float bias3 = w.fc3_b[0];
  double st[Rule::SUMS] = {};
  __syncthreads();

  const int64_t tiles = (a.B + 63) / 64;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t row0 = tile * 64;
    {
      const bool active = row0 + lane < a.B;
      int64_t i = active ? (a.index ? a.index[row0 + lane] : row0 + lane) : 0;
      i = i < 0 ? 0 : (i >= a.rows ? a.rows - 1 : i);  // never a read outside the storage
#pragma unroll
      for (int s = 0; s < Rule::SRC; ++s) src[s][lane] = active ? Rule::row(a, i, s) : nullptr;
      ys[lane] = active ? Rule::target(a, i, row0 + lane) : 0.0f;
    }
    __syncthreads();
    int col = 0;
#pragma unroll
    for (int s = 0; s < Rule::SRC; ++s) {
      if (!Rule::SKIP_EMPTY || in[s]) stage_rows(xs, kMgX, src[s], in[s], col, lane);
      col += in[s];
    }
    __syncthreads();

#pragma unroll 1
    for (int half = 0; half < 2; ++half) {
      const float* sv = lds_here(svec);
      mlp_grad_half(acc, rule.layer1(w1s), a2, a2t, sv, xs, ts, ds, ys, half, row0, a.B, bias3, a.g_scale, lane,
                    [&](float e, float y) { Rule::stat(st, e, y); });
    }
  }

  const MlpGradLayout Y(D, H, Rule::SUMS);
  mlp_grad_write(a.partials + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * Y.np, Y, acc, st, xs, red64, L1::ONES, D, H, lane);
}

// For the reduce kernels (256 threads, red: [256] doubles).  Workgroup blockIdx.x owns sixteen consecutive entries of the partial
// vectors: entry e of the result = the sum over the n_parts partial vectors of entry e, in float64 and in an order the grid alone
// fixes — sixteen slices of the partial vectors per entry, then a tree over the slices.  Returns e on the thread that holds the
// entry's sum in red[threadIdx.x], -1 on every other thread.
__device__ __forceinline__ int reduce16_entries(const double* partials, int n_parts, int np, int n_entries, double* red) {
  const int t = threadIdx.x, q = t & 15, s = t >> 4, e = 16 * blockIdx.x + q;
  const bool valid = e < n_entries;
  double sum = 0.0;
  if (valid)
    for (int p = s; p < n_parts; p += 16) sum += partials[(int64_t)p * np + e];
  red[t] = sum;
  __syncthreads();
  for (int w = 8; w >= 1; w >>= 1) {
    if (s < w) red[t] += red[t + 16 * w];
    __syncthreads();
  }
  return s == 0 && valid ? e : -1;
}

// which of the N tensors entry e belongs to (off: their N starts, then the sums': six tensors for PPO and TD3, eight for SAC)
template <int N>
__device__ __forceinline__ int entry_tensor(int e, const int32_t (&off)[N + 1]) {
  int k = 0;
#pragma unroll
  for (int j = 1; j < N; ++j)
    if (e >= off[j]) k = j;
  return k;
}

// A reduce kernel's gradient workgroup: reduce16_entries, then adjust(k, j, v) of the sum v of entry j of tensor k into grad[k][j].
template <class Adjust>
__device__ __forceinline__ void reduce16_store(const double* partials, int n_parts, int np, const int32_t (&off)[7], float* const* grad,
                                               double* red, Adjust&& adjust) {
  const int e = reduce16_entries(partials, n_parts, np, off[6], red);
  if (e < 0) return;
  const int k = entry_tensor<6>(e, off);
  float* dst = grad[0];
#pragma unroll
  for (int j = 1; j < 6; ++j)
    if (k == j) dst = grad[j];
  dst[e - off[k]] = (float)adjust(k, e - off[k], red[threadIdx.x]);
}

// the sum of `mine` over the workgroup's 256 threads (a tree), on every thread
__device__ __forceinline__ double block_tree(double* red, double mine) {
  const int t = threadIdx.x;
  __syncthreads();
  red[t] = mine;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }
  return red[0];
}

// the sum of one entry over the partial vectors (col: the entry in vector 0): 256 strided slices, then the tree
__device__ __forceinline__ double block_sum_column(const double* col, int n_parts, int np, double* red) {
  double mine = 0.0;
  for (int p = threadIdx.x; p < n_parts; p += 256) mine += col[(int64_t)p * np];
  return block_tree(red, mine);
}

}  // namespace qr
