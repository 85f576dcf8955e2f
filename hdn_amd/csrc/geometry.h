// What the geometry kernels share, each rule stated once: the sample point of the projective warp (warp_point) and of the log-polar sampler
// (logpolar_point), which the forwards (dlt_warp.hip, logpolar.hip) and their backwards (geometry_bwd.hip) both call, so a backward differentiates
// through exactly the taps its forward read; the DLT system and its elimination (dlt_elem, dlt_row, solve8); and what the backward kernels of
// geometry_bwd.hip and affine_stn.hip share (namespace gbwd).  The including files switch contraction off only after this header, so it does so
// itself, as hdn_common.h does around rn_mul: every operation below is rounded on its own, fusion is spelled __builtin_fmaf / fma.
#pragma once
#include <initializer_list>

#include "hdn_common.h"
#include "reduce.h"

#pragma clang fp contract(off)

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

// ------------------------------------------------------------------------------------------------ projective warp: one output pixel's sample point
struct WarpPoint {
  float gx, gy;        // the pixel's grid coordinates
  float t, xs, ys;     // the denominator after the nudge; x_s = T0 / t, y_s = T1 / t
  int x0, x1, y0, y1;  // the tap coordinates, clamped into the plane
  float ax, bx, ay, by;  // x1 - x, x - x0, y1 - y, y - y0: the CLAMPED taps against the UNCLAMPED coordinate (utils.py:181-184)
};

// Pixel (row i, column j) of an H x W output under theta th[9]; the arithmetic follows the reference's op order (utils.py:70-254).
__device__ __forceinline__ WarpPoint warp_point(const float* th, int i, int j, int H, int W) {
  WarpPoint p;
  p.gx = grid_coord(j, W), p.gy = grid_coord(i, H);
  // T = theta @ [gx, gy, 1]: fma(t1, gy, t0*gx) + t2   (the reference's sgemm order; utils.py:230)
  const float T0 = rn_add(__builtin_fmaf(th[1], p.gy, rn_mul(th[0], p.gx)), th[2]);
  const float T1 = rn_add(__builtin_fmaf(th[4], p.gy, rn_mul(th[3], p.gx)), th[5]);
  float t = rn_add(__builtin_fmaf(th[7], p.gy, rn_mul(th[6], p.gx)), th[8]);
  // utils.py:236-240: t += 1e-6 * (1 - [|t| >= 1e-7])
  t = rn_add(t, rn_mul(1e-6f, (fabsf(t) >= 1e-7f) ? 0.0f : 1.0f));
  p.t = t, p.xs = rn_div(T0, t), p.ys = rn_div(T1, t);
  // utils.py:128-129: x = (x_s + 1) * W / 2
  const float x = rn_mul(rn_mul(rn_add(p.xs, 1.0f), (float)W), 0.5f);
  const float y = rn_mul(rn_mul(rn_add(p.ys, 1.0f), (float)H), 0.5f);
  const int xf = f2i_x86(floorf(x)), yf = f2i_x86(floorf(y));
  p.x0 = clampi(xf, 0, W - 1), p.x1 = clampi((int)((unsigned)xf + 1u), 0, W - 1);
  p.y0 = clampi(yf, 0, H - 1), p.y1 = clampi((int)((unsigned)yf + 1u), 0, H - 1);
  p.ax = rn_sub((float)p.x1, x), p.bx = rn_sub(x, (float)p.x0), p.ay = rn_sub((float)p.y1, y), p.by = rn_sub(y, (float)p.y0);
  return p;
}

// ------------------------------------------------------------------------------------------------ log-polar sampler: one output pixel's sample point
struct LogpolarPoint {
  float gx, gy;        // the grid point (what the forward writes to `grid`)
  float pxu, pyu;      // the pixel position before the border clamp (the backward's border masks)
  float w, e, nn, s;   // w = px - floor(px), e = 1 - w, nn = py - floor(py), s = 1 - nn, of the clamped position
  int x0, y0, x1, y1;  // the taps; x1 = x0 and y1 = y0 where the east / south neighbour lies beyond the last index: always inside the plane
  bool e_ok, s_ok;     // does the east / south neighbour exist?  A tap that does not reads 0 and receives nothing
};

// Output pixel pix = a * S + b (a = angle row, b = log-radius column) of sample n; PyTorch's CPU grid_sampler step by step (logpolar.hip).
__device__ __forceinline__ LogpolarPoint logpolar_point(const float* __restrict__ polar, const float* __restrict__ rho,
                                                        const float* __restrict__ cosT, const float* __restrict__ sinT, int n, int pix, int H,
                                                        int W, int S) {
  LogpolarPoint p;
  const int a = pix / S, b = pix - a * S;
  const float r = rho[b];
  // logpolar.py:112-116: the x coordinate is divided by sz[2]//2 (= H//2), the y coordinate by sz[3]//2 (= W//2)  (sic)
  p.gx = rn_div(rn_add(rn_mul(r, cosT[a]), polar[2 * n]), (float)(H / 2));
  p.gy = rn_div(rn_add(rn_mul(r, sinT[a]), polar[2 * n + 1]), (float)(W / 2));
  p.pxu = rn_sub(rn_mul(rn_add(p.gx, 1.0f), rn_mul((float)W, 0.5f)), 0.5f);
  p.pyu = rn_sub(rn_mul(rn_add(p.gy, 1.0f), rn_mul((float)H, 0.5f)), 0.5f);
  const float px = fminf((float)(W - 1), fmaxf(0.0f, p.pxu));  // NaN -> 0, as the reference's clamp order does
  const float py = fminf((float)(H - 1), fmaxf(0.0f, p.pyu));
  const float xw = floorf(px), yn = floorf(py);
  p.w = rn_sub(px, xw), p.e = rn_sub(1.0f, p.w);
  p.nn = rn_sub(py, yn), p.s = rn_sub(1.0f, p.nn);
  p.x0 = (int)xw, p.y0 = (int)yn;
  p.e_ok = p.x0 + 1 < W, p.s_ok = p.y0 + 1 < H;
  p.x1 = p.e_ok ? p.x0 + 1 : p.x0, p.y1 = p.s_ok ? p.y0 + 1 : p.y0;
  return p;
}

// ------------------------------------------------------------------------------------------------ DLT: the 8 x 9 system and its elimination
// Row r of [A|b] of one sample (utils.py:7-67): row 2q is (x, y, 1, 0, 0, 0, -u x, -u y | u) and row 2q + 1 is (0, 0, 0, x, y, 1, -v x, -v y | v)
// of point dlt_point(q), (u, v) = src + off.  A row travels BY VALUE (Row9 in, Row9 out): handed on by reference the compiler keeps it in memory
// (18 KB of LDS per workgroup, or 35 more VGPRs) instead of the nine register pairs it gets this way.
struct Row9 {
  double v[9];
};
__device__ __forceinline__ Row9 dlt_row(const float* __restrict__ src, const float* __restrict__ off, int r) {
  Row9 row;
  double(&a)[9] = row.v;
  const int p = dlt_point(r >> 1);
  const double x = (double)src[2 * p], y = (double)src[2 * p + 1];
  // dst = src + off is an fp32 add in the reference (utils.py:36)
  const double u = (double)rn_add(src[2 * p], off[2 * p]);
  const double v = (double)rn_add(src[2 * p + 1], off[2 * p + 1]);
  if ((r & 1) == 0) {
    a[0] = x; a[1] = y; a[2] = 1.0; a[3] = 0.0; a[4] = 0.0; a[5] = 0.0; a[6] = -u * x; a[7] = -u * y; a[8] = u;
  } else {
    a[0] = 0.0; a[1] = 0.0; a[2] = 0.0; a[3] = x; a[4] = y; a[5] = 1.0; a[6] = -v * x; a[7] = -v * y; a[8] = v;
  }
  return row;
}

// Element (j, c) of the same [A|b] (c == 8: b), for the one place that walks a COLUMN of it: the backward's transposed system.
__device__ __forceinline__ double dlt_elem(const float* __restrict__ src, const float* __restrict__ off, int j, int c) {
  const int p = dlt_point(j >> 1);
  const double x = (double)src[2 * p], y = (double)src[2 * p + 1];
  const int k = 2 * p + (j & 1);
  const double d = (double)rn_add(src[k], off[k]);  // u on an even row, v on an odd one: an fp32 add in the reference (utils.py:36)
  const int c3 = (j & 1) ? c - 3 : c;                // the odd rows hold (x, y, 1) three columns further
  if (c == 8) return d;
  if (c == 6) return -d * x;
  if (c == 7) return -d * y;
  return c3 == 0 ? x : (c3 == 1 ? y : (c3 == 2 ? 1.0 : 0.0));
}

// Gauss-Jordan with partial pivoting on the 8 x 9 system whose row r = lane & 7 is `row`, in an aligned group of 8 lanes: pivot search and
// pivot-row broadcast are wave shuffles, so nothing touches memory.  Every lane of the wave calls it.  Returns the r-th unknown.
__device__ __forceinline__ double solve8(Row9 row, int r) {
  double(&a)[9] = row.v;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    // partial pivoting over rows >= k; ties resolve to the lowest row (as LAPACK's idamax does)
    double best = (r >= k) ? fabs(a[k]) : -1.0;
    int bidx = r;
#pragma unroll
    for (int m = 4; m >= 1; m >>= 1) {
      const double ob = __shfl_xor(best, m, 8);
      const int oi = __shfl_xor(bidx, m, 8);
      if (ob > best || (ob == best && oi < bidx)) { best = ob; bidx = oi; }
    }
    double prow[9], krow[9];
#pragma unroll
    for (int j = k; j < 9; ++j) {
      prow[j] = __shfl(a[j], bidx, 8);
      krow[j] = __shfl(a[j], k, 8);
    }
    if (r == k) {
#pragma unroll
      for (int j = k; j < 9; ++j) a[j] = prow[j];
    } else if (r == bidx) {
#pragma unroll
      for (int j = k; j < 9; ++j) a[j] = krow[j];
    }
    if (r != k) {
      const double f = a[k] / prow[k];
#pragma unroll
      for (int j = k; j < 9; ++j) a[j] = fma(-f, prow[j], a[j]);
    }
  }
  // after Gauss-Jordan row r is [0 .. a[r] .. 0 | a[8]]
  double diag = a[0];
#pragma unroll
  for (int j = 1; j < 8; ++j) diag = (r == j) ? a[j] : diag;
  return a[8] / diag;
}

// ------------------------------------------------------------------------------------------------ shared by the backward kernels
// (geometry_bwd.hip, affine_stn.hip): the per-channel loop of a bilinear sampler's backward, the second launch behind the deterministic parameter
// gradients (the first is block_sum_store of reduce.h) and the entry points' host sequence.
namespace gbwd {

// The four taps of one bilinear sample as its backward needs them.
struct Taps {
  int i_nw, i_ne, i_sw, i_se;   // y * W + x inside a plane: always a valid index
  bool k_nw, k_ne, k_sw, k_se;  // a tap that is not kept reads 0 and receives nothing
  float e, w, s, n;             // the weights' factors: nw = s e, ne = s w, sw = n e, se = n w
};

// One lane's walk over the C channels of its sample.  im / gi: the sample's image and grad_img (or NULL), planes `plane` floats apart; g: grad_out
// of this sample point at channel 0, channels `gstride` floats apart.  sums (kernel-uniform): add gout * d out / d px and gout * d out / d py over
// the channels, in ascending order, to dpx and dpy.  The loads are unconditional (the value is selected afterwards): a lane issues its four back to back.
__device__ __forceinline__ void channels_bwd(const Taps& t, const float* __restrict__ im, float* __restrict__ gi, size_t plane,
                                             const float* __restrict__ g, size_t gstride, int C, bool sums, float& dpx, float& dpy) {
  const float nw = rn_mul(t.s, t.e), ne = rn_mul(t.s, t.w), sw = rn_mul(t.n, t.e), se = rn_mul(t.n, t.w);
  for (int c = 0; c < C; ++c) {
    const float go = g[size_t(c) * gstride];
    if (sums) {
      const float* pl = im + c * plane;
      const float l_nw = pl[t.i_nw], l_ne = pl[t.i_ne], l_sw = pl[t.i_sw], l_se = pl[t.i_se];
      const float v_nw = t.k_nw ? l_nw : 0.f, v_ne = t.k_ne ? l_ne : 0.f, v_sw = t.k_sw ? l_sw : 0.f, v_se = t.k_se ? l_se : 0.f;
      const float dx = rn_add(rn_mul(t.s, rn_sub(v_ne, v_nw)), rn_mul(t.n, rn_sub(v_se, v_sw)));
      const float dy = rn_add(rn_mul(t.e, rn_sub(v_sw, v_nw)), rn_mul(t.w, rn_sub(v_se, v_ne)));
      dpx = rn_add(dpx, rn_mul(go, dx));
      dpy = rn_add(dpy, rn_mul(go, dy));
    }
    if (gi) {
      float* pl = gi + c * plane;
      if (t.k_nw) atomicAdd(pl + t.i_nw, rn_mul(go, nw));
      if (t.k_ne) atomicAdd(pl + t.i_ne, rn_mul(go, ne));
      if (t.k_sw) atomicAdd(pl + t.i_sw, rn_mul(go, sw));
      if (t.k_se) atomicAdd(pl + t.i_se, rn_mul(go, se));
    }
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
    s = wave_sum(s);
    if (lane == 0) out[b * N + q] = rn_mul(q == 0 ? s0 : s1, s);
  }
}

inline int zero_fill(float* p, long long floats, hipStream_t st) {
  return hip_status(hipMemsetAsync(p, 0, size_t(floats) * sizeof(float), st));
}

// an output may not be an input or the other output
inline bool aliases(const float* out, const float* const* others, int n) {
  for (int q = 0; q < n; ++q)
    if (out && out == others[q]) return true;
  return false;
}

// The host sequence of a sampler's backward once its pointers and shapes are checked: the workspace of the parameter gradient (N floats per
// (sample, block); asked for only when grad_par is), the alias rule over `inputs`, the zero fill of grad_img, launch(part) - the backward kernel on
// a grid of nblk x B, part = NULL when grad_par is - and the reduction of the partials, scaled by s0 (entry 0) and s1 (the rest).  img and grad_out,
// first and last of `inputs` (at most 6), are what the workspace may not overlap.  -> HDN_OK or the first error, in this order.
template <int N, class Launch>
inline int sampler_bwd(std::initializer_list<const float*> inputs, long long img_floats, long long out_floats, float* grad_par, float* grad_img,
                       float* workspace, long long workspace_bytes, long long need, int nblk, int B, float s0, float s1, hipStream_t st,
                       Launch launch) {
  float* part = nullptr;
  if (grad_par) {
    const int rc = check_workspace(workspace, workspace_bytes, need, *inputs.begin(), img_floats * 4, *(inputs.end() - 1), out_floats * 4);
    if (rc) return rc;
    part = workspace;
  }
  const float* ins[8];
  int n = 0;
  for (const float* p : inputs) ins[n++] = p;
  ins[n++] = part;
  ins[n++] = grad_img;
  if (aliases(grad_par, ins, n) || aliases(grad_img, ins, n - 1)) return HDN_E_ALIAS;
  if (grad_img) {
    const int rc = zero_fill(grad_img, img_floats, st);
    if (rc) return rc;
  }
  launch(part);
  if (part) hipLaunchKernelGGL(reduce_partials_kernel<N>, dim3(B), dim3(HDN_WAVE), 0, st, part, grad_par, nblk, s0, s1);
  return launch_status();
}

}  // namespace gbwd

}  // namespace hdn

#pragma clang fp contract(fast)
