// Shared device/host helpers for libhdn_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <atomic>

#include "../../include/hdn_hip.h"

#define HDN_WAVE 64
#define HDN_BLOCK 256

namespace hdn {

constexpr int cdiv(int a, int b) { return (a + b - 1) / b; }
constexpr int round_up(int a, int b) { return cdiv(a, b) * b; }

// One-time-per-device bookkeeping (hipFuncSetAttribute, device symbol addresses): the library assumes one process per
// GPU but stays correct when a process drives several devices.
// The entry points are reached through ctypes (GIL released), so two host threads can make their first call at the same
// time: the mask is atomic (a duplicated one-time call is harmless, a lost bit is not).  Device ids beyond 63 are never
// marked done and simply repeat the (cheap, idempotent) setup on every call.
struct PerDeviceOnce {
  std::atomic<unsigned long long> mask{0};
  static int device() {
    int d = 0;
    (void)hipGetDevice(&d);
    return d;
  }
  bool done(int d) const { return d >= 0 && d < 64 && ((mask.load(std::memory_order_acquire) >> d) & 1ull); }
  void set(int d) {
    if (d >= 0 && d < 64) mask.fetch_or(1ull << d, std::memory_order_release);
  }
};

// range_check.hip: HDN_OK, or HDN_E_LIMIT when an fp32 input of a two-fp16-piece kernel leaves fp16's range (HDN_CHECK_RANGE=1 /
// hdn_set_check_range; a no-op otherwise and inside stream captures)
int check_fp16_range(const float* x, long long n, hipStream_t stream, int act_domain = 0);   // act_domain 1: x is already x_real * 2^-8

// epilogue.hip: out[n] = [relu](slice 0 + slice 1 + ... + slice Z - 1 (+ bias[i % C])) of the K slices ws[Z][n], added in slice order (deterministic);
// bias may be NULL; n and C multiples of 4, everything 16-byte aligned.  The finish pass of the K-split forms of conv3x3s2.hip and conv3x3d.hip.
int finish_slices(const float* ws, int Z, const float* bias, int relu, float* out, long long n, int C, hipStream_t stream);

inline int hip_status(hipError_t e) { return e == hipSuccess ? HDN_OK : -(1000 + (int)e); }
inline int launch_status() { return hip_status(hipGetLastError()); }

// Dynamic LDS above 64 KiB needs an opt-in once per kernel and device: raises the limit of every kernel named to `bytes`, in argument order,
// unless `once` (a function-local static of the caller: one per template instantiation) says this device has been through it.
template <class... Kernels>
inline int lds_opt_in(PerDeviceOnce& once, int bytes, Kernels... kernels) {
  const int d = PerDeviceOnce::device();
  if (once.done(d)) return HDN_OK;
  for (const void* fn : {reinterpret_cast<const void*>(kernels)...})
    if (const int rc = hip_status(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes))) return rc;
  once.set(d);
  return HDN_OK;
}

// An integer switch of the environment: its value when it is set and positive, `fallback` otherwise.
inline int env_positive(const char* name, int fallback) {
  const char* e = getenv(name);
  const int v = e ? atoi(e) : 0;
  return v > 0 ? v : fallback;
}

// Copy n floats global -> LDS, linear image.  16-byte path when the source is aligned
// (always the case for whole-tensor torch allocations and full plane groups).
__device__ __forceinline__ void copy_g2l(const float* __restrict__ src, float* dst, int n, int tid) {
  if ((reinterpret_cast<uintptr_t>(src) & 15u) == 0) {
    const int n4 = n >> 2;
    const float4* s4 = reinterpret_cast<const float4*>(src);
    float4* d4 = reinterpret_cast<float4*>(dst);
    for (int i = tid; i < n4; i += HDN_BLOCK) d4[i] = s4[i];
    for (int i = (n4 << 2) + tid; i < n; i += HDN_BLOCK) dst[i] = src[i];
  } else {
    for (int i = tid; i < n; i += HDN_BLOCK) dst[i] = src[i];
  }
}

// Copy n floats LDS -> global, linear image.
__device__ __forceinline__ void copy_l2g(const float* src, float* __restrict__ dst, int n, int tid) {
  if ((reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
    const int n4 = n >> 2;
    const float4* s4 = reinterpret_cast<const float4*>(src);
    float4* d4 = reinterpret_cast<float4*>(dst);
    for (int i = tid; i < n4; i += HDN_BLOCK) d4[i] = s4[i];
    for (int i = (n4 << 2) + tid; i < n; i += HDN_BLOCK) dst[i] = src[i];
  } else {
    for (int i = tid; i < n; i += HDN_BLOCK) dst[i] = src[i];
  }
}

// Streaming hints for data that is touched exactly once (the correlation kernels' planes): nontemporal 16-byte loads / stores.
// tools/experiments/ubench_stream.hip: the 5x5 (x) 35x35 traffic shape 156.8 -> 148.5 us, the 5x5 (x) 29x29 shape 98.9 -> 75-89 us.
// HDN_STREAM_HINT: bit 0 = loads, bit 1 = stores (A/B switch; default both).
#ifndef HDN_STREAM_HINT
#define HDN_STREAM_HINT 3
#endif
typedef float hdn_f4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ld_stream(const float4* p) {
#if HDN_STREAM_HINT & 1
  const hdn_f4v v = __builtin_nontemporal_load(reinterpret_cast<const hdn_f4v*>(p));
  return float4{v.x, v.y, v.z, v.w};
#else
  return *p;
#endif
}
__device__ __forceinline__ void st_stream(float4* p, const float4& v) {
#if HDN_STREAM_HINT & 2
  __builtin_nontemporal_store(hdn_f4v{v.x, v.y, v.z, v.w}, reinterpret_cast<hdn_f4v*>(p));
#else
  *p = v;
#endif
}

// Same copy for a compile-time float count when the workgroup owns a full plane group: every thread issues ALL of
// its 16-byte loads before the first LDS write, so one HBM round trip covers the whole group (the runtime-count
// loop above gets serialised load -> wait -> write by the compiler).
template <int NFLOATS>
__device__ __forceinline__ void copy_g2l_full(const float* __restrict__ src, float* dst, int tid) {
  static_assert(NFLOATS % 4 == 0, "plane groups are multiples of 4 floats");
  constexpr int N4 = NFLOATS / 4;
  constexpr int ITER = cdiv(N4, HDN_BLOCK);
  const float4* s4 = reinterpret_cast<const float4*>(src);
  float4* d4 = reinterpret_cast<float4*>(dst);
  float4 r[ITER];
#pragma unroll
  for (int q = 0; q < ITER; ++q) r[q] = ld_stream(s4 + min(tid + q * HDN_BLOCK, N4 - 1));  // unconditional: stays in registers
#pragma unroll
  for (int q = 0; q < ITER; ++q) {
    const int i = tid + q * HDN_BLOCK;
    if (i < N4) d4[i] = r[q];
  }
}

template <int NFLOATS>
__device__ __forceinline__ void copy_l2g_full(const float* src, float* __restrict__ dst, int tid) {
  static_assert(NFLOATS % 4 == 0, "plane groups are multiples of 4 floats");
  constexpr int N4 = NFLOATS / 4;
  constexpr int ITER = cdiv(N4, HDN_BLOCK);
  const float4* s4 = reinterpret_cast<const float4*>(src);
  float4* d4 = reinterpret_cast<float4*>(dst);
#pragma unroll
  for (int q = 0; q < ITER; ++q) {
    const int i = tid + q * HDN_BLOCK;
    if (i < N4) st_stream(d4 + i, s4[i]);
  }
}

// Individually rounded fp32 operations.  In this toolchain __fmul_rn/__fadd_rn/... are plain operators compiled under
// the default -ffp-contract=fast, so `__fadd_rn(__fmul_rn(a, b), c)` may still become one fma.  These helpers are
// compiled with contraction off: a product feeding a sum stays two roundings, as in the reference's CPU kernels.
#pragma clang fp contract(off)
__device__ __forceinline__ float rn_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float rn_add(float a, float b) { return a + b; }
__device__ __forceinline__ float rn_sub(float a, float b) { return a - b; }
__device__ __forceinline__ float rn_div(float a, float b) { return a / b; }  // IEEE-correct (v_div_scale/fmas/fixup)
#pragma clang fp contract(fast)

__host__ __device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// do the byte ranges [a, a + na) and [b, b + nb) intersect? (the entry points' HDN_E_ALIAS checks)
inline bool bytes_overlap(const void* a, long long na, const void* b, long long nb) {
  const char *pa = static_cast<const char*>(a), *pb = static_cast<const char*>(b);
  return pa < pb + nb && pb < pa + na;
}

// an operand of an entry point as a byte range (p NULL: absent)
struct Range {
  const void* p;
  long long bytes;
};

// does any of the first n_out ranges (the outputs) overlap another range of the list?
inline bool any_output_overlaps(const Range* r, int n_out, int n) {
  for (int i = 0; i < n_out; ++i) {
    if (!r[i].p) continue;
    for (int j = i + 1; j < n; ++j)
      if (r[j].p && bytes_overlap(r[i].p, r[i].bytes, r[j].p, r[j].bytes)) return true;
  }
  return false;
}

// the entry points' checks of a K-slice workspace of `need` bytes (need <= 0: none is used, nothing is checked) beside the input x and the output:
// NULL -> HDN_E_NULL, unaligned or too small -> HDN_E_LIMIT, overlapping x or out -> HDN_E_ALIAS, in that order
inline int check_workspace(const void* ws, long long ws_bytes, long long need, const void* x, long long x_bytes, const void* out, long long out_bytes) {
  if (need <= 0) return HDN_OK;
  if (!ws) return HDN_E_NULL;
  if (!aligned16(ws) || ws_bytes < need) return HDN_E_LIMIT;
  if (bytes_overlap(ws, need, x, x_bytes) || bytes_overlap(ws, need, out, out_bytes)) return HDN_E_ALIAS;
  return HDN_OK;
}

typedef float float2v __attribute__((ext_vector_type(2)));

// LDS byte address of a __shared__ pointer (low 32 bits of the flat address are the LDS offset).
__device__ __forceinline__ uint32_t lds_addr(const void* p) { return static_cast<uint32_t>(reinterpret_cast<uintptr_t>(p)); }

// One ds_read2_b32: the pair (lds[addr + 4*O0], lds[addr + 4*O1]) lands in an aligned VGPR pair, ready to be a
// v_pk_fma_f32 operand.  Issued through inline asm so that LLVM cannot merge the two halves with other loads of
// the same dwords and rebuild the pair with v_mov (which it does for the C++ form).  The load is NOT tracked by
// the compiler's s_waitcnt insertion: consume only after lds_wait_all().
template <int O0, int O1>
__device__ __forceinline__ float2v lds_read_pair(uint32_t addr) {
  static_assert(O0 >= 0 && O0 < 256 && O1 >= 0 && O1 < 256, "ds_read2_b32 offsets are 8-bit dword counts");
  float2v r;
  asm volatile("ds_read2_b32 %0, %1 offset0:%2 offset1:%3" : "=v"(r) : "v"(addr), "n"(O0), "n"(O1) : "memory");
  return r;
}

__device__ __forceinline__ void lds_wait_all() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// Make `v` opaque at this point so no consumer of it can be scheduled above (cdna guide §5.7 item 3).
__device__ __forceinline__ void pin(float2v& v) { asm volatile("" : "+v"(v)); }

}  // namespace hdn
