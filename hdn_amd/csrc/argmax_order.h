// The argmax order of the similarity branch's head maps, stated once: similarity.hip (the tracker's decode) and simi_geometry.hip (the training
// forward's picks) both include this file.  tests/test_gpu_simi_decode.py is the guard of the order.
#pragma once
#include <math.h>

#include "hdn_common.h"

#pragma clang fp contract(off)

namespace hdn {

// softmax(1)[:, 1] of a 2-class logit pair as ATen's vectorised CPU kernel forms it: exp(x - max) for both, times 1 / sum.
__device__ __forceinline__ float softmax2_class1(float x0, float x1) {
  const float m = fmaxf(x0, x1);
  const float e0 = expf(rn_sub(x0, m)), e1 = expf(rn_sub(x1, m));
  return rn_mul(e1, rn_div(1.0f, rn_add(e0, e1)));
}

// np.argmax's order on (value, index) candidates: a NaN is above every number, then the larger value, then - among equals and among
// NaNs - the lower index.  True when candidate (ov, oi) replaces (v, i).
__device__ __forceinline__ bool argmax_takes(double ov, int oi, double v, int i) {
  const bool on = ov != ov, vn = v != v;
  if (on || vn) return on && (!vn || oi < i);
  return ov > v || (ov == v && oi < i);
}

// The cell a lane starts from: its own first cell, or - an idle lane of a map smaller than the wave - cell 0 once more.  No lane holds a
// sentinel: whatever the butterfly keeps is a cell of the map, and the duplicate of cell 0 ties with lane 0's own (same value, same index).
__device__ __forceinline__ int argmax_start(int lane, int n) { return lane < n ? lane : 0; }

__device__ __forceinline__ void wave_argmax(double& v, int& i) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const double ov = __shfl_xor(v, s);
    const int oi = __shfl_xor(i, s);
    if (argmax_takes(ov, oi, v, i)) { v = ov; i = oi; }
  }
}

}  // namespace hdn
