// Index and coordinate helpers that the geometry kernels share: the forward (dlt_warp.hip) and its backward (geometry_bwd.hip) must pick the same
// points, grid coordinates and taps, so both take them from here; and what the backward kernels of geometry_bwd.hip and affine_stn.hip share (namespace
// gbwd).  Nothing below uses a bare fp32 operator: the roundings are those of rn_* and
// __builtin_fmaf whatever contraction mode the including file compiles under.
#pragma once
#include "hdn_common.h"

namespace hdn {

constexpr int WARP_PX_PER_THREAD = 4;
constexpr int WARP_PX_PER_BLOCK = HDN_BLOCK * WARP_PX_PER_THREAD;

// reference point order inside the solve: utils.py:18-26 gathers columns [0,1,2,3,6,7,4,5]
__device__ __forceinline__ int dlt_point(int p) { return p == 2 ? 3 : (p == 3 ? 2 : p); }

// torch.linspace(-1, 1, n)[i] on the CPU: start + step*i below the midpoint, end - step*(n-1-i)
// above, each with a single rounding (verified bit-for-bit in tests/test_host_logic.py).
__device__ __forceinline__ float grid_coord(int i, int n) {
  const float step = rn_div(2.0f, (float)(n - 1));
  return i < n / 2 ? __builtin_fmaf(step, (float)i, -1.0f) : __builtin_fmaf(-step, (float)(n - 1 - i), 1.0f);
}

// float -> int32 as the reference's x86 path converts it: out-of-range and NaN give INT_MIN.
__device__ __forceinline__ int f2i_x86(float f) {
  return (f >= -2147483648.0f && f < 2147483648.0f) ? (int)f : (int)0x80000000;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ------------------------------------------------------------------------------------------------ shared by the backward kernels
// (geometry_bwd.hip, affine_stn.hip): the fixed-order reductions behind the deterministic parameter gradients and the entry points' helpers.
namespace gbwd {

constexpr int WAVES = HDN_BLOCK / HDN_WAVE;

// v[q] summed over the block in a fixed order; thread q < N then writes the sum to dst[q].  lds: WAVES * N floats.  Every thread of the block calls it.
template <int N>
__device__ __forceinline__ void block_sum_store(float (&v)[N], float* lds, float* __restrict__ dst) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int q = 0; q < N; ++q) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v[q] = rn_add(v[q], __shfl_xor(v[q], m, HDN_WAVE));
  }
  if ((tid & (HDN_WAVE - 1)) == 0) {
#pragma unroll
    for (int q = 0; q < N; ++q) lds[(tid >> 6) * N + q] = v[q];
  }
  __syncthreads();
  if (tid < N) {
    float s = lds[tid];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) s = rn_add(s, lds[w * N + tid]);
    dst[tid] = s;
  }
}

// out[b][q] = scale[q] * (partials part[b][0 .. nblk)[q] added in a fixed order); one wave per sample.
template <int N>
__global__ __launch_bounds__(HDN_WAVE) void reduce_partials_kernel(const float* __restrict__ part, float* __restrict__ out, int nblk, const float s0,
                                                                    const float s1) {
  const size_t b = blockIdx.x;
  const int lane = threadIdx.x;
  const float* p = part + b * nblk * N;
#pragma unroll
  for (int q = 0; q < N; ++q) {
    float s = 0.f;
    for (int k = lane; k < nblk; k += HDN_WAVE) s = rn_add(s, p[size_t(k) * N + q]);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s = rn_add(s, __shfl_xor(s, m, HDN_WAVE));
    if (lane == 0) out[b * N + q] = rn_mul(q == 0 ? s0 : s1, s);
  }
}

inline int zero_fill(float* p, long long floats, hipStream_t st) {
  const hipError_t e = hipMemsetAsync(p, 0, size_t(floats) * sizeof(float), st);
  return e == hipSuccess ? HDN_OK : -(1000 + (int)e);
}

// an output may not be an input or the other output
inline bool aliases(const float* out, const float* const* others, int n) {
  for (int q = 0; q < n; ++q)
    if (out && out == others[q]) return true;
  return false;
}

}  // namespace gbwd

}  // namespace hdn
