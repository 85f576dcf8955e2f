// Index and coordinate helpers that the geometry kernels share: the forward (dlt_warp.hip) and its backward (geometry_bwd.hip) must pick the same
// points, grid coordinates and taps, so both take them from here.  Nothing below uses a bare fp32 operator: the roundings are those of rn_* and
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

}  // namespace hdn
