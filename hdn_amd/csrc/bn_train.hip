// BatchNorm2d on batch statistics (+ ReLU) for training, forward and backward, for gfx950: hdn_bn_relu_train_fwd_f32 / hdn_bn_relu_train_bwd_f32.
// The formulas, the layouts and the checks are in include/hdn_hip.h.
//
// c (and dc) is channels-last, [N = B P][C] row-major.  A workgroup of HDN_BLOCK threads owns a SLICE of 32 channels: thread t holds the channel quad
// cq = t & 7 (one float4) of the rows r, r + 32, ... with r = t >> 3, so a wave's access covers eight whole 128-byte row segments.  The NCHW side (y or
// dy with layout flag 1) goes through a padded LDS tile of 32 channels x 64 pixels: on that side thread t holds pixel t & 63 of the channels t >> 6,
// t >> 6 + 4, ..., lanes run along pixels (dword accesses: a plane with odd P starts at 4-byte alignment only), and every pixel derives its own
// (image, position), so a tile may straddle images.  Leading dimension 65: a quad-side access lands on bank (4 cq + j + r) mod 32, which is distinct
// within each 32-lane half (4 cq in 0 .. 28, four rows) and repeats across the halves; that costs nothing only because the LDS serves a dword
// access half a wave at a time (the guides' bank model; not measured here).  The pixel-side accesses are consecutive.
//
// z = (c - mean) alpha + beta is stated ONCE, bn_z below: subtract first (a folded c alpha + (beta - mean alpha) loses 2^-24 |mean| alpha of z), then one
// explicit fmaf.  Forward and backward both call it and the backward recomputes the ReLU mask from c: the two directions see the same mask bit for bit.
//
// Sums over pixels are float64 from the product on (c c and dz x^ are exact in float64) and deterministic, without atomics: a thread adds its rows in
// ascending order; the 32 row-threads of a channel are added by reduce.h's wave_sum after a transposition through LDS (lane = row-thread); in the split
// form every workgroup writes its 64 sums as one partial to the workspace and the finish launch adds the partials l, l + 64, ... in lane l, then
// wave_sum.  The order depends on (B, P, C) and the form only.
//
// Forms (hdn_bn_relu_train_form): 0, N <= FUSED_MAX_ROWS: ONE launch of C / 32 workgroups, each through statistics and normalisation of its slice (the
//   second pass re-reads its 128 N bytes from L2); no workspace.
// 1: partial sums over (C / 32) x chunks workgroups, a finish of C / 32 workgroups, apply over the same grid.  docs/KERNELS.md has the measurements.
#include "hdn_common.h"
#include "reduce.h"

namespace hdn {
namespace bnt {

constexpr int SLICE = 32;                 // channels of a workgroup
constexpr int ROWS = HDN_BLOCK / 8;       // rows of one pass of the workgroup
constexpr int TILE = 64;                  // pixels of the LDS tile
constexpr int TLD = TILE + 1;             // its leading dimension, floats
constexpr int RLD = 2 * SLICE + 1;        // leading dimension of the reduction's transposition, doubles
constexpr int FUSED_MAX_ROWS = 400;       // form 0 up to this N (docs/KERNELS.md, "BatchNorm + ReLU in training")
constexpr int TARGET_WGS = 1024;          // form 1: about this many workgroups per launch

struct Smem {
  float tile[SLICE * TLD];
  double red[ROWS * RLD];
  double tot[2 * SLICE];
  float mean[SLICE], invstd[SLICE];
};

// ------------------------------------------------------------------------------------------------------------ the one statement of z
__device__ __forceinline__ float bn_alpha(float gamma, float invstd) { return rn_mul(gamma, invstd); }
__device__ __forceinline__ float bn_z(float c, float mean, float alpha, float beta) { return __builtin_fmaf(rn_sub(c, mean), alpha, beta); }
// relu that keeps a NaN (fmaxf would drop it)
__device__ __forceinline__ float bn_act(float z, int relu) { return (relu && z < 0.f) ? 0.f : z; }
// dz = dy [z > 0]
__device__ __forceinline__ float bn_dz(float z, float dy, int relu) { return (relu && !(z > 0.f)) ? 0.f : dy; }
__device__ __forceinline__ float bn_xhat(float c, float mean, float invstd) { return rn_mul(rn_sub(c, mean), invstd); }

struct Ch4 {  // the four channels of a thread
  float mean[4], invstd[4], alpha[4], beta[4];
};

__device__ __forceinline__ void load_ch4(Ch4& k, const float* mean, const float* invstd, const float* __restrict__ gamma, const float* __restrict__ beta,
                                         int ch) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    k.mean[j] = mean[j];
    k.invstd[j] = invstd[j];
    k.alpha[j] = bn_alpha(gamma[ch + j], invstd[j]);
    k.beta[j] = beta[ch + j];
  }
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float at(const float4& v, int j) { return j == 0 ? v.x : (j == 1 ? v.y : (j == 2 ? v.z : v.w)); }

// ------------------------------------------------------------------------------------------------------------ reductions
// v[2 j + kind] of every thread (its channel quad) summed over the 32 row-threads: s.tot[2 (channel of the slice) + kind], then a barrier.
__device__ __forceinline__ void slice_sum(const double (&v)[8], Smem& s) {
  const int tid = threadIdx.x, cq = tid & 7, r = tid >> 3;
#pragma unroll
  for (int i = 0; i < 8; ++i) s.red[r * RLD + cq * 8 + i] = v[i];
  __syncthreads();
  const int l = lane_id(), w = wave_id();
  double keep = 0.0;
#pragma unroll
  for (int j = 0; j < 2 * SLICE / BLOCK_WAVES; ++j) {
    const double x = wave_sum(l < ROWS ? s.red[l * RLD + w * (2 * SLICE / BLOCK_WAVES) + j] : 0.0);
    if (l == j) keep = x;
  }
  if (l < 2 * SLICE / BLOCK_WAVES) s.tot[w * (2 * SLICE / BLOCK_WAVES) + l] = keep;
  __syncthreads();
}

// the partials part[chunk][C][2] of the slice at ch0 added over the chunks: s.tot as above, then a barrier
__device__ __forceinline__ void partial_sum(const double* __restrict__ part, int nchunks, int C, int ch0, Smem& s) {
  const int l = lane_id(), w = wave_id();
  double keep = 0.0;
#pragma unroll 1
  for (int j = 0; j < 2 * SLICE / BLOCK_WAVES; ++j) {
    const int q = w * (2 * SLICE / BLOCK_WAVES) + j;
    double x = 0.0;
    for (int k = l; k < nchunks; k += HDN_WAVE) x = fixed_add(x, part[(size_t(k) * C + ch0) * 2 + q]);
    x = wave_sum(x);
    if (l == j) keep = x;
  }
  if (l < 2 * SLICE / BLOCK_WAVES) s.tot[w * (2 * SLICE / BLOCK_WAVES) + l] = keep;
  __syncthreads();
}

__device__ __forceinline__ void store_partial(const Smem& s, double* __restrict__ part, int chunk, int C, int ch0) {
  if (threadIdx.x < 2 * SLICE) part[(size_t(chunk) * C + ch0) * 2 + threadIdx.x] = s.tot[threadIdx.x];
}

// thread t < 32, channel ch0 + t: mean / invstd from s.tot into `stats` and s.mean / s.invstd, the running buffers advanced; then a barrier
__device__ __forceinline__ void finish_stats(Smem& s, float* __restrict__ stats, float* __restrict__ rmean, float* __restrict__ rvar, double momentum,
                                             double eps, double n, int C, int ch0) {
  const int t = threadIdx.x;
  if (t < SLICE) {
    const double mean = s.tot[2 * t] / n;
    double var = s.tot[2 * t + 1] / n - mean * mean;
    var = var < 0.0 ? 0.0 : var;  // (a NaN stays a NaN)
    const float mean_f = (float)mean, invstd_f = (float)(1.0 / sqrt(var + eps));
    stats[ch0 + t] = mean_f;
    stats[C + ch0 + t] = invstd_f;
    s.mean[t] = mean_f;
    s.invstd[t] = invstd_f;
    if (rmean) rmean[ch0 + t] = (float)((1.0 - momentum) * (double)rmean[ch0 + t] + momentum * mean);
    if (rvar) rvar[ch0 + t] = (float)((1.0 - momentum) * (double)rvar[ch0 + t] + momentum * (var * (n / (n - 1.0))));
  }
  __syncthreads();
}

// ------------------------------------------------------------------------------------------------------------ passes over rows [n_lo, n_hi)
__device__ __forceinline__ void acc_fwd(const float* __restrict__ c, int C, int ch, int n_lo, int n_hi, double (&v)[8]) {
#pragma unroll 4
  for (int n = n_lo + (threadIdx.x >> 3); n < n_hi; n += ROWS) {
    const float4 x = ld4(c + size_t(n) * C + ch);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double d = (double)at(x, j);
      v[2 * j] += d;
      v[2 * j + 1] += d * d;
    }
  }
}

template <bool NCHW>
__device__ __forceinline__ void apply_fwd(const float* __restrict__ c, float* __restrict__ y, float* tile, const Ch4& k, int C, int P, int ch0, int n_lo,
                                          int n_hi, int relu) {
  const int tid = threadIdx.x, cq = tid & 7, r = tid >> 3;
  for (int n0 = n_lo; n0 < n_hi; n0 += TILE) {
#pragma unroll
    for (int h = 0; h < TILE / ROWS; ++h) {
      const int row = r + ROWS * h, n = n0 + row;
      if (n < n_hi) {
        const float4 x = ld4(c + size_t(n) * C + ch0 + 4 * cq);
        float z[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) z[j] = bn_act(bn_z(at(x, j), k.mean[j], k.alpha[j], k.beta[j]), relu);
        if (NCHW) {
#pragma unroll
          for (int j = 0; j < 4; ++j) tile[(4 * cq + j) * TLD + row] = z[j];
        } else {
          *reinterpret_cast<float4*>(y + size_t(n) * C + ch0 + 4 * cq) = make_float4(z[0], z[1], z[2], z[3]);
        }
      }
    }
    if (NCHW) {
      __syncthreads();
      const int px = tid & (TILE - 1), n = n0 + px;
      if (n < n_hi) {
        const int b = n / P, p = n - b * P;
        float* yp = y + (size_t(b) * C + ch0) * P + p;
#pragma unroll
        for (int q = 0; q < SLICE / BLOCK_WAVES; ++q) {
          const int ch = (tid >> 6) + BLOCK_WAVES * q;
          yp[size_t(ch) * P] = tile[ch * TLD + px];
        }
      }
      __syncthreads();
    }
  }
}

// dy of the tile at n0 for this thread's rows and channel quad (zeros beyond n_hi)
template <bool NCHW>
__device__ __forceinline__ void load_dy(const float* __restrict__ dy, float* tile, int C, int P, int ch0, int n0, int n_hi, float4 (&g)[TILE / ROWS]) {
  const int tid = threadIdx.x, cq = tid & 7, r = tid >> 3;
  if (NCHW) {
    const int px = tid & (TILE - 1), n = n0 + px;
    if (n < n_hi) {
      const int b = n / P, p = n - b * P;
      const float* dp = dy + (size_t(b) * C + ch0) * P + p;
#pragma unroll
      for (int q = 0; q < SLICE / BLOCK_WAVES; ++q) {
        const int ch = (tid >> 6) + BLOCK_WAVES * q;
        tile[ch * TLD + px] = dp[size_t(ch) * P];
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int h = 0; h < TILE / ROWS; ++h) {
    const int row = r + ROWS * h, n = n0 + row;
    g[h] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (n < n_hi) {
      if (NCHW)
        g[h] = make_float4(tile[(4 * cq) * TLD + row], tile[(4 * cq + 1) * TLD + row], tile[(4 * cq + 2) * TLD + row], tile[(4 * cq + 3) * TLD + row]);
      else
        g[h] = ld4(dy + size_t(n) * C + ch0 + 4 * cq);
    }
  }
  if (NCHW) __syncthreads();
}

// v[2 j] += dz, v[2 j + 1] += dz x^
template <bool NCHW>
__device__ __forceinline__ void acc_bwd(const float* __restrict__ dy, const float* __restrict__ c, float* tile, const Ch4& k, int C, int P, int ch0,
                                        int n_lo, int n_hi, int relu, double (&v)[8]) {
  const int tid = threadIdx.x, cq = tid & 7, r = tid >> 3;
  for (int n0 = n_lo; n0 < n_hi; n0 += TILE) {
    float4 g[TILE / ROWS];
    load_dy<NCHW>(dy, tile, C, P, ch0, n0, n_hi, g);
#pragma unroll
    for (int h = 0; h < TILE / ROWS; ++h) {
      const int n = n0 + r + ROWS * h;
      if (n < n_hi) {
        const float4 x = ld4(c + size_t(n) * C + ch0 + 4 * cq);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float cv = at(x, j);
          const float dz = bn_dz(bn_z(cv, k.mean[j], k.alpha[j], k.beta[j]), at(g[h], j), relu);
          v[2 * j] += (double)dz;
          v[2 * j + 1] += (double)dz * (double)bn_xhat(cv, k.mean[j], k.invstd[j]);
        }
      }
    }
  }
}

// dc = alpha (dz - m1 - x^ m2), m1 = S1 / N, m2 = S2 / N
template <bool NCHW>
__device__ __forceinline__ void apply_bwd(const float* __restrict__ dy, const float* __restrict__ c, float* __restrict__ dc, float* tile, const Ch4& k,
                                          const float (&m1)[4], const float (&m2)[4], int C, int P, int ch0, int n_lo, int n_hi, int relu) {
  const int tid = threadIdx.x, cq = tid & 7, r = tid >> 3;
  for (int n0 = n_lo; n0 < n_hi; n0 += TILE) {
    float4 g[TILE / ROWS];
    load_dy<NCHW>(dy, tile, C, P, ch0, n0, n_hi, g);
#pragma unroll
    for (int h = 0; h < TILE / ROWS; ++h) {
      const int n = n0 + r + ROWS * h;
      if (n < n_hi) {
        const float4 x = ld4(c + size_t(n) * C + ch0 + 4 * cq);
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float cv = at(x, j);
          const float dz = bn_dz(bn_z(cv, k.mean[j], k.alpha[j], k.beta[j]), at(g[h], j), relu);
          const float xh = bn_xhat(cv, k.mean[j], k.invstd[j]);
          o[j] = rn_mul(k.alpha[j], rn_sub(rn_sub(dz, m1[j]), rn_mul(xh, m2[j])));
        }
        *reinterpret_cast<float4*>(dc + size_t(n) * C + ch0 + 4 * cq) = make_float4(o[0], o[1], o[2], o[3]);
      }
    }
  }
}

// thread t < 32: S1, S2 of channel ch0 + t from s.tot into dbeta / dgamma (where asked) and S1 / N, S2 / N into m1[t], m2[t]
__device__ __forceinline__ void finish_grads(const double* tot, float* __restrict__ dgamma, float* __restrict__ dbeta, int ch0, float* m1, float* m2,
                                             double n) {
  const int t = threadIdx.x;
  if (t < SLICE) {
    const double s1 = tot[2 * t], s2 = tot[2 * t + 1];
    if (dbeta) dbeta[ch0 + t] = (float)s1;
    if (dgamma) dgamma[ch0 + t] = (float)s2;
    m1[t] = (float)(s1 / n);
    m2[t] = (float)(s2 / n);
  }
}

// ------------------------------------------------------------------------------------------------------------ kernels
// form 0
template <bool NCHW>
__global__ __launch_bounds__(HDN_BLOCK) void fwd_fused_kernel(const float* __restrict__ c, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              float* __restrict__ y, float* __restrict__ stats, float* __restrict__ rmean,
                                                              float* __restrict__ rvar, double momentum, double eps, int N, int P, int C, int relu) {
  __shared__ Smem s;
  const int ch0 = blockIdx.x * SLICE, cq = threadIdx.x & 7;
  double v[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  acc_fwd(c, C, ch0 + 4 * cq, 0, N, v);
  slice_sum(v, s);
  finish_stats(s, stats, rmean, rvar, momentum, eps, (double)N, C, ch0);
  Ch4 k;
  load_ch4(k, s.mean + 4 * cq, s.invstd + 4 * cq, gamma, beta, ch0 + 4 * cq);
  apply_fwd<NCHW>(c, y, s.tile, k, C, P, ch0, 0, N, relu);
}

template <bool NCHW>
__global__ __launch_bounds__(HDN_BLOCK) void bwd_fused_kernel(const float* __restrict__ dy, const float* __restrict__ c, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, const float* __restrict__ stats, float* __restrict__ dc,
                                                              float* __restrict__ dgamma, float* __restrict__ dbeta, int N, int P, int C, int relu) {
  __shared__ Smem s;
  const int ch0 = blockIdx.x * SLICE, cq = threadIdx.x & 7, ch = ch0 + 4 * cq;
  Ch4 k;
  load_ch4(k, stats + ch, stats + C + ch, gamma, beta, ch);
  double v[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  acc_bwd<NCHW>(dy, c, s.tile, k, C, P, ch0, 0, N, relu, v);
  slice_sum(v, s);
  finish_grads(s.tot, dgamma, dbeta, ch0, s.mean, s.invstd, (double)N);   // S1 / N, S2 / N in s.mean, s.invstd
  if (!dc) return;  // kernel-uniform
  __syncthreads();
  float m1[4], m2[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    m1[j] = s.mean[4 * cq + j];
    m2[j] = s.invstd[4 * cq + j];
  }
  apply_bwd<NCHW>(dy, c, dc, s.tile, k, m1, m2, C, P, ch0, 0, N, relu);
}

// form 1: blockIdx.x = slice, blockIdx.y = chunk of `rpw` rows
__global__ __launch_bounds__(HDN_BLOCK) void fwd_partial_kernel(const float* __restrict__ c, double* __restrict__ part, int N, int C, int rpw) {
  __shared__ Smem s;
  const int ch0 = blockIdx.x * SLICE, n_lo = blockIdx.y * rpw, n_hi = min(N, n_lo + rpw);
  double v[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  acc_fwd(c, C, ch0 + 4 * (threadIdx.x & 7), n_lo, n_hi, v);
  slice_sum(v, s);
  store_partial(s, part, blockIdx.y, C, ch0);
}

__global__ __launch_bounds__(HDN_BLOCK) void fwd_finish_kernel(const double* __restrict__ part, int nchunks, float* __restrict__ stats,
                                                               float* __restrict__ rmean, float* __restrict__ rvar, double momentum, double eps, double n,
                                                               int C) {
  __shared__ Smem s;
  const int ch0 = blockIdx.x * SLICE;
  partial_sum(part, nchunks, C, ch0, s);
  finish_stats(s, stats, rmean, rvar, momentum, eps, n, C, ch0);
}

template <bool NCHW>
__global__ __launch_bounds__(HDN_BLOCK) void fwd_apply_kernel(const float* __restrict__ c, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              const float* __restrict__ stats, float* __restrict__ y, int N, int P, int C, int rpw,
                                                              int relu) {
  __shared__ float tile[NCHW ? SLICE * TLD : 1];
  const int ch0 = blockIdx.x * SLICE, ch = ch0 + 4 * (threadIdx.x & 7), n_lo = blockIdx.y * rpw, n_hi = min(N, n_lo + rpw);
  Ch4 k;
  load_ch4(k, stats + ch, stats + C + ch, gamma, beta, ch);
  apply_fwd<NCHW>(c, y, tile, k, C, P, ch0, n_lo, n_hi, relu);
}

template <bool NCHW>
__global__ __launch_bounds__(HDN_BLOCK) void bwd_partial_kernel(const float* __restrict__ dy, const float* __restrict__ c, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, const float* __restrict__ stats,
                                                                double* __restrict__ part, int N, int P, int C, int rpw, int relu) {
  __shared__ Smem s;
  const int ch0 = blockIdx.x * SLICE, ch = ch0 + 4 * (threadIdx.x & 7), n_lo = blockIdx.y * rpw, n_hi = min(N, n_lo + rpw);
  Ch4 k;
  load_ch4(k, stats + ch, stats + C + ch, gamma, beta, ch);
  double v[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  acc_bwd<NCHW>(dy, c, s.tile, k, C, P, ch0, n_lo, n_hi, relu, v);
  slice_sum(v, s);
  store_partial(s, part, blockIdx.y, C, ch0);
}

// m: the head of the workspace, S1 / N [C], S2 / N [C]
__global__ __launch_bounds__(HDN_BLOCK) void bwd_finish_kernel(const double* __restrict__ part, int nchunks, float* __restrict__ dgamma,
                                                               float* __restrict__ dbeta, float* __restrict__ m, double n, int C) {
  __shared__ Smem s;
  const int ch0 = blockIdx.x * SLICE;
  partial_sum(part, nchunks, C, ch0, s);
  finish_grads(s.tot, dgamma, dbeta, ch0, m + ch0, m + C + ch0, n);
}

template <bool NCHW>
__global__ __launch_bounds__(HDN_BLOCK) void bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ c, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, const float* __restrict__ stats, const float* __restrict__ m,
                                                              float* __restrict__ dc, int N, int P, int C, int rpw, int relu) {
  __shared__ float tile[NCHW ? SLICE * TLD : 1];
  const int ch0 = blockIdx.x * SLICE, ch = ch0 + 4 * (threadIdx.x & 7), n_lo = blockIdx.y * rpw, n_hi = min(N, n_lo + rpw);
  Ch4 k;
  load_ch4(k, stats + ch, stats + C + ch, gamma, beta, ch);
  float m1[4], m2[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    m1[j] = m[ch + j];
    m2[j] = m[C + ch + j];
  }
  apply_bwd<NCHW>(dy, c, dc, tile, k, m1, m2, C, P, ch0, n_lo, n_hi, relu);
}

// ------------------------------------------------------------------------------------------------------------ host
struct Plan {
  int form, rpw, nchunks;
  long long ws_bytes;
};

static int check_shape(int B, int P, int C) {
  if (B <= 0 || P <= 0 || C <= 0 || C % SLICE != 0) return HDN_E_SHAPE;
  if ((long long)B * P < 2) return HDN_E_SHAPE;
  if (C > 2048 || (long long)B * P * C > 0x7fffffffLL) return HDN_E_LIMIT;
  return HDN_OK;
}

// valid (B, P, C) only.  HDN_BN_TRAIN_FUSED_ROWS: the threshold between the forms, for the A/B runs of tools/head_bn_train_bench.py
static Plan make_plan(int B, int P, int C) {
  const int N = B * P;
  Plan p;
  if (N <= env_positive("HDN_BN_TRAIN_FUSED_ROWS", FUSED_MAX_ROWS)) {
    p.form = 0, p.rpw = N, p.nchunks = 1, p.ws_bytes = 0;
    return p;
  }
  const int target = TARGET_WGS / (C / SLICE) > 0 ? TARGET_WGS / (C / SLICE) : 1;
  p.form = 1;
  p.rpw = round_up(cdiv(N, target), TILE);
  p.nchunks = cdiv(N, p.rpw);
  p.ws_bytes = 2LL * C * (long long)sizeof(float) + 2LL * p.nchunks * C * (long long)sizeof(double);
  return p;
}

}  // namespace bnt
}  // namespace hdn

extern "C" {

long long hdn_bn_relu_train_workspace_bytes(int B, int P, int C) {
  const int rc = hdn::bnt::check_shape(B, P, C);
  return rc ? rc : hdn::bnt::make_plan(B, P, C).ws_bytes;
}

int hdn_bn_relu_train_form(int B, int P, int C) {
  const int rc = hdn::bnt::check_shape(B, P, C);
  return rc ? rc : hdn::bnt::make_plan(B, P, C).form;
}

int hdn_bn_relu_train_fwd_f32(const float* c, const float* gamma, const float* beta, float* y, float* stats, float* running_mean_or_null,
                              float* running_var_or_null, double momentum, double eps, void* ws, long long ws_bytes, int B, int P, int C, int relu,
                              int y_layout, void* stream) {
  using namespace hdn;
  using namespace hdn::bnt;
  if (!c || !gamma || !beta || !y || !stats) return HDN_E_NULL;
  if (B <= 0 || P <= 0 || C <= 0 || C % SLICE != 0 || (long long)B * P < 2) return HDN_E_SHAPE;
  if ((relu != 0 && relu != 1) || (y_layout != 0 && y_layout != 1)) return HDN_E_SHAPE;
  if (!(eps > 0.0) || !(momentum >= 0.0 && momentum <= 1.0)) return HDN_E_SHAPE;
  if (const int rc = check_shape(B, P, C)) return rc;
  const Plan p = make_plan(B, P, C);
  if (p.ws_bytes && !ws) return HDN_E_NULL;
  if (!aligned16(c) || (y_layout == 0 && !aligned16(y)) || (p.ws_bytes && (!aligned16(ws) || ws_bytes < p.ws_bytes))) return HDN_E_LIMIT;
  const int N = B * P;
  const long long nb = (long long)N * C * 4;
  const Range r[8] = {{y, nb},   {stats, 2LL * C * 4}, {running_mean_or_null, C * 4LL}, {running_var_or_null, C * 4LL}, {p.ws_bytes ? ws : nullptr, p.ws_bytes},
                      {c, nb},   {gamma, C * 4LL},     {beta, C * 4LL}};
  if (any_output_overlaps(r, 5, 8)) return HDN_E_ALIAS;

  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 slices(C / SLICE), grid(C / SLICE, p.nchunks), block(HDN_BLOCK);
  if (p.form == 0) {
    if (y_layout)
      hipLaunchKernelGGL(fwd_fused_kernel<true>, slices, block, 0, st, c, gamma, beta, y, stats, running_mean_or_null, running_var_or_null, momentum, eps, N,
                         P, C, relu);
    else
      hipLaunchKernelGGL(fwd_fused_kernel<false>, slices, block, 0, st, c, gamma, beta, y, stats, running_mean_or_null, running_var_or_null, momentum, eps,
                         N, P, C, relu);
    return launch_status();
  }
  double* part = reinterpret_cast<double*>(static_cast<float*>(ws) + 2 * C);
  hipLaunchKernelGGL(fwd_partial_kernel, grid, block, 0, st, c, part, N, C, p.rpw);
  hipLaunchKernelGGL(fwd_finish_kernel, slices, block, 0, st, (const double*)part, p.nchunks, stats, running_mean_or_null, running_var_or_null, momentum, eps,
                     (double)N, C);
  if (y_layout)
    hipLaunchKernelGGL(fwd_apply_kernel<true>, grid, block, 0, st, c, gamma, beta, (const float*)stats, y, N, P, C, p.rpw, relu);
  else
    hipLaunchKernelGGL(fwd_apply_kernel<false>, grid, block, 0, st, c, gamma, beta, (const float*)stats, y, N, P, C, p.rpw, relu);
  return launch_status();
}

int hdn_bn_relu_train_bwd_f32(const float* dy, const float* c, const float* gamma, const float* beta, const float* stats, float* dc_or_null,
                              float* dgamma_or_null, float* dbeta_or_null, void* ws, long long ws_bytes, int B, int P, int C, int relu, int dy_layout,
                              void* stream) {
  using namespace hdn;
  using namespace hdn::bnt;
  if (!dy || !c || !gamma || !beta || !stats) return HDN_E_NULL;
  if (B <= 0 || P <= 0 || C <= 0 || C % SLICE != 0 || (long long)B * P < 2) return HDN_E_SHAPE;
  if ((relu != 0 && relu != 1) || (dy_layout != 0 && dy_layout != 1)) return HDN_E_SHAPE;
  if (!dc_or_null && !dgamma_or_null && !dbeta_or_null) return HDN_E_SHAPE;
  if (const int rc = check_shape(B, P, C)) return rc;
  const Plan p = make_plan(B, P, C);
  if (p.ws_bytes && !ws) return HDN_E_NULL;
  if (!aligned16(c) || !aligned16(dc_or_null) || (dy_layout == 0 && !aligned16(dy)) || (p.ws_bytes && (!aligned16(ws) || ws_bytes < p.ws_bytes)))
    return HDN_E_LIMIT;
  const int N = B * P;
  const long long nb = (long long)N * C * 4;
  const Range r[9] = {{dc_or_null, nb}, {dgamma_or_null, C * 4LL}, {dbeta_or_null, C * 4LL}, {p.ws_bytes ? ws : nullptr, p.ws_bytes}, {dy, nb}, {c, nb},
                      {gamma, C * 4LL}, {beta, C * 4LL},           {stats, 2LL * C * 4}};
  if (any_output_overlaps(r, 4, 9)) return HDN_E_ALIAS;

  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 slices(C / SLICE), grid(C / SLICE, p.nchunks), block(HDN_BLOCK);
  if (p.form == 0) {
    if (dy_layout)
      hipLaunchKernelGGL(bwd_fused_kernel<true>, slices, block, 0, st, dy, c, gamma, beta, stats, dc_or_null, dgamma_or_null, dbeta_or_null, N, P, C, relu);
    else
      hipLaunchKernelGGL(bwd_fused_kernel<false>, slices, block, 0, st, dy, c, gamma, beta, stats, dc_or_null, dgamma_or_null, dbeta_or_null, N, P, C, relu);
    return launch_status();
  }
  float* m = static_cast<float*>(ws);
  double* part = reinterpret_cast<double*>(m + 2 * C);
  if (dy_layout)
    hipLaunchKernelGGL(bwd_partial_kernel<true>, grid, block, 0, st, dy, c, gamma, beta, stats, part, N, P, C, p.rpw, relu);
  else
    hipLaunchKernelGGL(bwd_partial_kernel<false>, grid, block, 0, st, dy, c, gamma, beta, stats, part, N, P, C, p.rpw, relu);
  hipLaunchKernelGGL(bwd_finish_kernel, slices, block, 0, st, (const double*)part, p.nchunks, dgamma_or_null, dbeta_or_null, m, (double)N, C);
  if (dc_or_null) {
    if (dy_layout)
      hipLaunchKernelGGL(bwd_apply_kernel<true>, grid, block, 0, st, dy, c, gamma, beta, stats, (const float*)m, dc_or_null, N, P, C, p.rpw, relu);
    else
      hipLaunchKernelGGL(bwd_apply_kernel<false>, grid, block, 0, st, dy, c, gamma, beta, stats, (const float*)m, dc_or_null, N, P, C, p.rpw, relu);
  }
  return launch_status();
}

}  // extern "C"
