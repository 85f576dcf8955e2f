// Fixed-order reductions over a wave and over a workgroup (gfx950, 64 lanes): the one statement of the kernels' determinism contract.
//
// Order.  A wave combines its 64 lanes in a xor butterfly with the masks 32, 16, ..., 1, which leaves the same bits in every lane.  A workgroup
// then combines its wave results in ascending wave order through LDS, one slot per wave: ((w0 + w1) + w2) + ...  An fp32 add is rn_add, a
// float64 or integer add is `+` compiled with contraction off: no add below ever becomes an fma, whatever the including file compiles under.
// There are no float atomics, so the same input gives the same bits on every call.
//
// Barriers.  Every thread of the workgroup calls a block_* helper, under uniform control flow.
//   block_sum, block_max: barrier, lane 0 of each wave writes its slot, barrier, every thread reads.  Two calls in a row on one scratch need
//     nothing from the caller.  There is NO barrier after the read: a caller that writes the scratch by other means, or publishes something else
//     through LDS, places its own __syncthreads().
//   block_sum_store: write, ONE barrier, threads q < N read and store.  A caller that reuses the scratch afterwards synchronises first.
#pragma once
#include "hdn_common.h"

namespace hdn {

constexpr int BLOCK_WAVES = HDN_BLOCK / HDN_WAVE;  // of a workgroup of HDN_BLOCK threads

__device__ __forceinline__ int lane_id() { return threadIdx.x & (HDN_WAVE - 1); }
__device__ __forceinline__ int wave_id() { return threadIdx.x / HDN_WAVE; }

// the add of the contract
__device__ __forceinline__ float fixed_add(float a, float b) { return rn_add(a, b); }
template <typename T>
__device__ __forceinline__ T fixed_add(T a, T b) {
#pragma clang fp contract(off)
  return a + b;
}

// float, double, int, unsigned; every lane gets the sum
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int m = HDN_WAVE / 2; m >= 1; m >>= 1) v = fixed_add(v, __shfl_xor(v, m, HDN_WAVE));
  return v;
}

// every lane gets the maximum.  float: NaN-free input (fmaxf drops a NaN, it does not carry it)
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int m = HDN_WAVE / 2; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, HDN_WAVE));
  return v;
}
__device__ __forceinline__ unsigned wave_max(unsigned v) {
#pragma unroll
  for (int m = HDN_WAVE / 2; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m, HDN_WAVE));
  return v;
}

// v[q] summed over a workgroup of WAVES waves, q < N at once: every thread gets every sum.  lds: WAVES * N values.
template <int WAVES, int N, typename T>
__device__ __forceinline__ void block_sum(T (&v)[N], T* lds) {
#pragma unroll
  for (int q = 0; q < N; ++q) v[q] = wave_sum(v[q]);
  __syncthreads();
  if (lane_id() == 0) {
#pragma unroll
    for (int q = 0; q < N; ++q) lds[wave_id() * N + q] = v[q];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < N; ++q) {
    v[q] = lds[q];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) v[q] = fixed_add(v[q], lds[w * N + q]);
  }
}

// one value: every thread returns the sum.  lds: WAVES values.
template <int WAVES, typename T>
__device__ __forceinline__ T block_sum(T v, T* lds) {
  T a[1] = {v};
  block_sum<WAVES>(a, lds);
  return a[0];
}

// every thread returns the maximum over the workgroup (NaN-free input).  lds: WAVES floats.
template <int WAVES>
__device__ __forceinline__ float block_max(float v, float* lds) {
  v = wave_max(v);
  __syncthreads();
  if (lane_id() == 0) lds[wave_id()] = v;
  __syncthreads();
  float t = lds[0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) t = fmaxf(t, lds[w]);
  return t;
}

// v[q] summed over the workgroup; thread q < N then writes the sum to dst[q * stride].  lds: WAVES * N values.
template <int N, int WAVES, typename T>
__device__ __forceinline__ void block_sum_store(T (&v)[N], T* lds, T* __restrict__ dst, size_t stride = 1) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int q = 0; q < N; ++q) v[q] = wave_sum(v[q]);
  if (lane_id() == 0) {
#pragma unroll
    for (int q = 0; q < N; ++q) lds[wave_id() * N + q] = v[q];
  }
  __syncthreads();
  if (tid < N) {
    T s = lds[tid];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) s = fixed_add(s, lds[w * N + tid]);
    dst[size_t(tid) * stride] = s;
  }
}

}  // namespace hdn
