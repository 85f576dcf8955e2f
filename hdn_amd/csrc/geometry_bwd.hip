// Backward of the three geometry operators for gfx950 (training only): hdn_logpolar_sample_bwd_f32 (logpolar.hip), hdn_dlt_solve_bwd_f32 and
// hdn_warp_bwd_f32 (dlt_warp.hip).  The formulas are in include/hdn_hip.h.
//
// Each kernel recomputes its forward's sample point with the forward's own statements (the same rn_* helpers, contraction off, the shared helpers of
// geometry.h), so the taps it differentiates through are the taps the forward read.  The launch shapes are the forward's: HDN_BLOCK threads, one
// pixel per lane in the sampler, WARP_PX_PER_THREAD per thread in the warp, one 8-lane group per sample in the solve.
//
// grad_polar / grad_theta (a sum over every pixel and channel of a sample) are deterministic and use no atomics: a lane adds its channels (and, in
// the warp, its pixels) in ascending order, a wave adds its lanes in a fixed xor tree (32 .. 1), the block's waves are added in ascending order through
// LDS (block_sum_store, geometry.h) and written as one partial per (sample, block) into the caller's workspace; reduce_partials_kernel (geometry.h), a second launch of the same call, has one
// wave per sample add the partials (lane l takes blocks l, l + 64, ... in ascending order, then the same tree).  Nothing depends on the batch size:
// sample b of a batch has the bits of that sample run alone.
// grad_img is a scatter: plain fp32 atomicAdd (one global_atomic_add_f32) into the buffer that the call zero-fills on the stream first.  The order in
// which colliding taps arrive is not fixed, so grad_img is NOT bit-reproducible between calls on arbitrary data.
#include "geometry.h"

#pragma clang fp contract(off)

namespace hdn {
namespace gbwd {

// ---------------------------------------------------------------------------------------------------------------- log-polar sampler
__global__ __launch_bounds__(HDN_BLOCK) void logpolar_bwd_kernel(const float* __restrict__ img, const float* __restrict__ polar,
                                                                 const float* __restrict__ rho, const float* __restrict__ cosT,
                                                                 const float* __restrict__ sinT, const float* __restrict__ gout,
                                                                 float* __restrict__ part, float* __restrict__ gimg, int C, int H, int W, int S) {
  __shared__ float red[WAVES * 2];
  const int n = blockIdx.y;
  const int pix = blockIdx.x * HDN_BLOCK + threadIdx.x;
  float acc[2] = {0.f, 0.f};  // sum over channels of gout * d out / d px, d out / d py, times the border rule
  if (pix < S * S) {
    // ---- the statements of logpolar_kernel ----
    const int a = pix / S, b = pix - a * S;
    const float r = rho[b];
    const float gx = rn_div(rn_add(rn_mul(r, cosT[a]), polar[2 * n]), (float)(H / 2));
    const float gy = rn_div(rn_add(rn_mul(r, sinT[a]), polar[2 * n + 1]), (float)(W / 2));
    const float pxu = rn_sub(rn_mul(rn_add(gx, 1.0f), rn_mul((float)W, 0.5f)), 0.5f);
    const float pyu = rn_sub(rn_mul(rn_add(gy, 1.0f), rn_mul((float)H, 0.5f)), 0.5f);
    const float px = fminf((float)(W - 1), fmaxf(0.0f, pxu));
    const float py = fminf((float)(H - 1), fmaxf(0.0f, pyu));
    const float xw = floorf(px), yn = floorf(py);
    const float w = rn_sub(px, xw), e = rn_sub(1.0f, w);
    const float nn = rn_sub(py, yn), s = rn_sub(1.0f, nn);
    const float nw = rn_mul(s, e), ne = rn_mul(s, w), sw = rn_mul(nn, e), se = rn_mul(nn, w);
    const int x0 = (int)xw, y0 = (int)yn;
    const bool e_ok = x0 + 1 < W, s_ok = y0 + 1 < H;
    const int x1 = e_ok ? x0 + 1 : x0, y1 = s_ok ? y0 + 1 : y0;
    // ---- clip_coordinates_set_grad: a coordinate that the clamp moved (or that sits on the border) has derivative 0 ----
    const float mx = (pxu <= 0.0f || pxu >= (float)(W - 1)) ? 0.f : 1.f;
    const float my = (pyu <= 0.0f || pyu >= (float)(H - 1)) ? 0.f : 1.f;
    const size_t HW = size_t(H) * W, SS = size_t(S) * S;
    const float* im = img + size_t(n) * C * HW;
    const float* g = gout + size_t(n) * C * SS + pix;
    float* gi = gimg ? gimg + size_t(n) * C * HW : nullptr;
    for (int c = 0; c < C; ++c) {
      const float go = g[size_t(c) * SS];
      if (part) {
        const float* pl = im + c * HW;
        const float v_nw = pl[y0 * W + x0];
        const float v_ne = e_ok ? pl[y0 * W + x1] : 0.f;
        const float v_sw = s_ok ? pl[y1 * W + x0] : 0.f;
        const float v_se = (e_ok && s_ok) ? pl[y1 * W + x1] : 0.f;
        const float dpx = rn_add(rn_mul(s, rn_sub(v_ne, v_nw)), rn_mul(nn, rn_sub(v_se, v_sw)));
        const float dpy = rn_add(rn_mul(e, rn_sub(v_sw, v_nw)), rn_mul(w, rn_sub(v_se, v_ne)));
        acc[0] = rn_add(acc[0], rn_mul(go, dpx));
        acc[1] = rn_add(acc[1], rn_mul(go, dpy));
      }
      if (gi) {
        float* pl = gi + c * HW;
        atomicAdd(pl + y0 * W + x0, rn_mul(go, nw));
        if (e_ok) atomicAdd(pl + y0 * W + x1, rn_mul(go, ne));
        if (s_ok) atomicAdd(pl + y1 * W + x0, rn_mul(go, sw));
        if (e_ok && s_ok) atomicAdd(pl + y1 * W + x1, rn_mul(go, se));
      }
    }
    acc[0] = rn_mul(acc[0], mx);
    acc[1] = rn_mul(acc[1], my);
  }
  if (part) block_sum_store<2>(acc, red, part + (size_t(n) * gridDim.x + blockIdx.x) * 2);  // kernel-uniform branch
}

// ---------------------------------------------------------------------------------------------------------------- DLT solve
// Element (j, c) of [A|b] (c == 8: b) of one sample, rows as dlt_solve_rows builds them.
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

// Gauss-Jordan with partial pivoting on the 8 x 9 system whose row r = lane & 7 is a[0..8], in an aligned group of 8 lanes: the elimination of
// dlt_solve_rows (dlt_warp.hip).  Every lane of the wave calls it.  Returns the r-th unknown.
__device__ __forceinline__ double solve8(double (&a)[9], int r) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {
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
  double diag = a[0];
#pragma unroll
  for (int j = 1; j < 8; ++j) diag = (r == j) ? a[j] : diag;
  return a[8] / diag;
}

__global__ __launch_bounds__(HDN_BLOCK) void dlt_solve_bwd_kernel(const float* __restrict__ src, const float* __restrict__ off,
                                                                  const float* __restrict__ gH, float* __restrict__ gsrc,
                                                                  float* __restrict__ goff, int B) {
  const int gid = (blockIdx.x * HDN_BLOCK + threadIdx.x) >> 3;
  const int b = min(gid, B - 1);  // keep every lane in the shuffles
  const int r = threadIdx.x & 7;
  const float* s = src + size_t(b) * 8;
  const float* o = off + size_t(b) * 8;
  double a[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) a[c] = dlt_elem(s, o, r, c);
  const double h = solve8(a, r);  // A h = b
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] = dlt_elem(s, o, j, r);  // row r of A^T
  a[8] = (double)gH[size_t(b) * 9 + r];                     // gH[8] meets the constant 1
  const double lam = solve8(a, r);  // A^T lambda = grad_h;  grad_b = lambda, grad_A = -lambda h^T
  double hc[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) hc[c] = __shfl(h, c, 8);
  const int p = dlt_point(r >> 1);
  const bool odd = r & 1;
  const double x = (double)s[2 * p], y = (double)s[2 * p + 1];
  const double d = (double)rn_add(s[2 * p + odd], o[2 * p + odd]);  // u (even row) or v (odd row)
  // row (x, y, 1, 0, 0, 0, -d x, -d y | d), its first three entries at columns 3..5 on an odd row
  const double gA6 = -lam * hc[6], gA7 = -lam * hc[7];
  const double gx = -lam * (odd ? hc[3] : hc[0]) - gA6 * d;
  const double gy = -lam * (odd ? hc[4] : hc[1]) - gA7 * d;
  const double gd = lam - gA6 * x - gA7 * y;                         // grad_u or grad_v
  const double ox = __shfl_xor(gx, 1, 8), oy = __shfl_xor(gy, 1, 8);  // the point's other row (every lane shuffles)
  const double gxy = odd ? gy + oy : gx + ox;                         // grad_x on the even lane, grad_y on the odd
  if (gid < B) {
    const size_t at = size_t(b) * 8 + 2 * p + odd;
    if (goff) goff[at] = (float)gd;
    if (gsrc) gsrc[at] = (float)(gxy + gd);
  }
}

// ---------------------------------------------------------------------------------------------------------------- projective warp
__global__ __launch_bounds__(HDN_BLOCK) void warp_bwd_kernel(const float* __restrict__ img, const float* __restrict__ theta,
                                                             const float* __restrict__ gout, float* __restrict__ part,
                                                             float* __restrict__ gimg, int C, int H, int W) {
  __shared__ float red[WAVES * 9];
  const int b = blockIdx.y;
  const size_t HW = size_t(H) * W;
  float th[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) th[q] = theta[size_t(b) * 9 + q];
  const float* im = img + size_t(b) * C * HW;
  const float* gb = gout + size_t(b) * C * HW;
  float* gi = gimg ? gimg + size_t(b) * C * HW : nullptr;
  float acc[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) acc[q] = 0.f;
  const int base = blockIdx.x * WARP_PX_PER_BLOCK + threadIdx.x;
#pragma unroll
  for (int q = 0; q < WARP_PX_PER_THREAD; ++q) {
    const int pix = base + q * HDN_BLOCK;
    if (pix >= H * W) continue;
    const int i = pix / W, j = pix - i * W;
    // ---- the statements of warp_pixel ----
    const float gx = grid_coord(j, W), gy = grid_coord(i, H);
    const float T0 = rn_add(__builtin_fmaf(th[1], gy, rn_mul(th[0], gx)), th[2]);
    const float T1 = rn_add(__builtin_fmaf(th[4], gy, rn_mul(th[3], gx)), th[5]);
    float t = rn_add(__builtin_fmaf(th[7], gy, rn_mul(th[6], gx)), th[8]);
    t = rn_add(t, rn_mul(1e-6f, (fabsf(t) >= 1e-7f) ? 0.0f : 1.0f));
    const float xs = rn_div(T0, t), ys = rn_div(T1, t);
    const float x = rn_mul(rn_mul(rn_add(xs, 1.0f), (float)W), 0.5f);
    const float y = rn_mul(rn_mul(rn_add(ys, 1.0f), (float)H), 0.5f);
    const int xf = f2i_x86(floorf(x)), yf = f2i_x86(floorf(y));
    const int x0 = clampi(xf, 0, W - 1), x1 = clampi((int)((unsigned)xf + 1u), 0, W - 1);
    const int y0 = clampi(yf, 0, H - 1), y1 = clampi((int)((unsigned)yf + 1u), 0, H - 1);
    const float x0f = (float)x0, x1f = (float)x1, y0f = (float)y0, y1f = (float)y1;
    const float ax = rn_sub(x1f, x), bx = rn_sub(x, x0f), ay = rn_sub(y1f, y), by = rn_sub(y, y0f);
    // ---- the integer taps are constants; the nudge has derivative 1 ----
    const float* g = gb + size_t(pix) * C;
    float sx = 0.f, sy = 0.f;  // sum over channels of gout * d out / d x, d out / d y
    for (int c = 0; c < C; ++c) {
      const float go = g[c];
      if (part) {
        const float* pl = im + c * HW;
        const float Ia = pl[y0 * W + x0], Ib = pl[y1 * W + x0], Ic = pl[y0 * W + x1], Id = pl[y1 * W + x1];
        const float dx = rn_add(rn_mul(rn_sub(Ic, Ia), ay), rn_mul(rn_sub(Id, Ib), by));
        const float dy = rn_add(rn_mul(rn_sub(Ib, Ia), ax), rn_mul(rn_sub(Id, Ic), bx));
        sx = rn_add(sx, rn_mul(go, dx));
        sy = rn_add(sy, rn_mul(go, dy));
      }
      if (gi) {
        float* pl = gi + c * HW;
        atomicAdd(pl + y0 * W + x0, rn_mul(go, rn_mul(ax, ay)));  // wa
        atomicAdd(pl + y1 * W + x0, rn_mul(go, rn_mul(ax, by)));  // wb
        atomicAdd(pl + y0 * W + x1, rn_mul(go, rn_mul(bx, ay)));  // wc
        atomicAdd(pl + y1 * W + x1, rn_mul(go, rn_mul(bx, by)));  // wd
      }
    }
    if (part) {
      // x = (xs + 1) W / 2, xs = T0 / t:  d x / d T0 = (W/2) / t,  d x / d t = -(W/2) xs / t
      const float gxs = rn_mul(sx, rn_mul((float)W, 0.5f)), gys = rn_mul(sy, rn_mul((float)H, 0.5f));
      const float g0 = rn_div(gxs, t), g1 = rn_div(gys, t);
      const float g2 = -rn_div(rn_add(rn_mul(gxs, xs), rn_mul(gys, ys)), t);
      // T_r = theta[3r] gx + theta[3r+1] gy + theta[3r+2]
      acc[0] = rn_add(acc[0], rn_mul(g0, gx)); acc[1] = rn_add(acc[1], rn_mul(g0, gy)); acc[2] = rn_add(acc[2], g0);
      acc[3] = rn_add(acc[3], rn_mul(g1, gx)); acc[4] = rn_add(acc[4], rn_mul(g1, gy)); acc[5] = rn_add(acc[5], g1);
      acc[6] = rn_add(acc[6], rn_mul(g2, gx)); acc[7] = rn_add(acc[7], rn_mul(g2, gy)); acc[8] = rn_add(acc[8], g2);
    }
  }
  if (part) block_sum_store<9>(acc, red, part + (size_t(b) * gridDim.x + blockIdx.x) * 9);  // kernel-uniform branch
}

}  // namespace gbwd
}  // namespace hdn

extern "C" {

long long hdn_logpolar_sample_bwd_workspace_bytes(int B, int S) {
  if (B <= 0 || S <= 0) return HDN_E_SHAPE;
  if (B > 65535 || (long long)S * S > (1LL << 30)) return HDN_E_LIMIT;
  return (long long)B * hdn::cdiv(S * S, HDN_BLOCK) * 2 * sizeof(float);
}

long long hdn_warp_bwd_workspace_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 1 || W <= 1) return HDN_E_SHAPE;
  if (B > 65535 || (long long)H * W > (1LL << 30)) return HDN_E_LIMIT;
  return (long long)B * hdn::cdiv(H * W, hdn::WARP_PX_PER_BLOCK) * 9 * sizeof(float);
}

int hdn_logpolar_sample_bwd_f32(const float* img, const float* polar, const float* rho, const float* cos_theta, const float* sin_theta,
                                const float* grad_out, float* grad_polar_or_null, float* grad_img_or_null, float* workspace,
                                long long workspace_bytes, int B, int C, int H, int W, int S, void* stream) {
  using namespace hdn;
  if (!img || !polar || !rho || !cos_theta || !sin_theta || !grad_out) return HDN_E_NULL;
  if (B <= 0 || C <= 0 || H <= 1 || W <= 1 || S <= 0 || (!grad_polar_or_null && !grad_img_or_null)) return HDN_E_SHAPE;
  if (B > 65535 || (long long)H * W > (1LL << 30) || (long long)S * S > (1LL << 30)) return HDN_E_LIMIT;
  const long long img_floats = (long long)B * C * H * W, out_floats = (long long)B * C * S * S;
  float* part = nullptr;
  if (grad_polar_or_null) {
    const int rc = check_workspace(workspace, workspace_bytes, hdn_logpolar_sample_bwd_workspace_bytes(B, S), img, img_floats * 4, grad_out,
                                   out_floats * 4);
    if (rc) return rc;
    part = workspace;
  }
  const float* ins[8] = {img, polar, rho, cos_theta, sin_theta, grad_out, part, grad_img_or_null};
  if (gbwd::aliases(grad_polar_or_null, ins, 8) || gbwd::aliases(grad_img_or_null, ins, 7)) return HDN_E_ALIAS;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (grad_img_or_null) {
    const int rc = gbwd::zero_fill(grad_img_or_null, img_floats, st);
    if (rc) return rc;
  }
  const int nblk = cdiv(S * S, HDN_BLOCK);
  hipLaunchKernelGGL(gbwd::logpolar_bwd_kernel, dim3(nblk, B), dim3(HDN_BLOCK), 0, st, img, polar, rho, cos_theta, sin_theta, grad_out, part,
                     grad_img_or_null, C, H, W, S);
  if (part) {
    // d px / d polar_x = (W/2) / (H//2), d py / d polar_y = (H/2) / (W//2): the forward's (sic) pairing
    const float fx = (float)W * 0.5f / (float)(H / 2), fy = (float)H * 0.5f / (float)(W / 2);
    hipLaunchKernelGGL(gbwd::reduce_partials_kernel<2>, dim3(B), dim3(HDN_WAVE), 0, st, part, grad_polar_or_null, nblk, fx, fy);
  }
  return launch_status();
}

int hdn_dlt_solve_bwd_f32(const float* src, const float* off, const float* grad_H, float* grad_src_or_null, float* grad_off_or_null, int B,
                          void* stream) {
  using namespace hdn;
  if (!src || !off || !grad_H) return HDN_E_NULL;
  if (B <= 0 || (!grad_src_or_null && !grad_off_or_null)) return HDN_E_SHAPE;
  if (B > (1 << 24)) return HDN_E_LIMIT;
  const float* ins[4] = {src, off, grad_H, grad_off_or_null};
  if (gbwd::aliases(grad_src_or_null, ins, 4) || gbwd::aliases(grad_off_or_null, ins, 3)) return HDN_E_ALIAS;
  hipLaunchKernelGGL(gbwd::dlt_solve_bwd_kernel, dim3(cdiv(B, HDN_BLOCK / 8)), dim3(HDN_BLOCK), 0, static_cast<hipStream_t>(stream), src, off,
                     grad_H, grad_src_or_null, grad_off_or_null, B);
  return launch_status();
}

int hdn_warp_bwd_f32(const float* img, const float* theta, const float* grad_out, float* grad_theta_or_null, float* grad_img_or_null,
                     float* workspace, long long workspace_bytes, int B, int C, int H, int W, void* stream) {
  using namespace hdn;
  if (!img || !theta || !grad_out) return HDN_E_NULL;
  if (B <= 0 || C <= 0 || H <= 1 || W <= 1 || (!grad_theta_or_null && !grad_img_or_null)) return HDN_E_SHAPE;
  if (B > 65535 || (long long)H * W > (1LL << 30) || (long long)C * H * W > 0x7fffffffLL) return HDN_E_LIMIT;
  const long long img_floats = (long long)B * C * H * W;
  float* part = nullptr;
  if (grad_theta_or_null) {
    const int rc = check_workspace(workspace, workspace_bytes, hdn_warp_bwd_workspace_bytes(B, H, W), img, img_floats * 4, grad_out, img_floats * 4);
    if (rc) return rc;
    part = workspace;
  }
  const float* ins[5] = {img, theta, grad_out, part, grad_img_or_null};
  if (gbwd::aliases(grad_theta_or_null, ins, 5) || gbwd::aliases(grad_img_or_null, ins, 4)) return HDN_E_ALIAS;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (grad_img_or_null) {
    const int rc = gbwd::zero_fill(grad_img_or_null, img_floats, st);
    if (rc) return rc;
  }
  const int nblk = cdiv(H * W, WARP_PX_PER_BLOCK);
  hipLaunchKernelGGL(gbwd::warp_bwd_kernel, dim3(nblk, B), dim3(HDN_BLOCK), 0, st, img, theta, grad_out, part, grad_img_or_null, C, H, W);
  if (part) hipLaunchKernelGGL(gbwd::reduce_partials_kernel<9>, dim3(B), dim3(HDN_WAVE), 0, st, part, grad_theta_or_null, nblk, 1.0f, 1.0f);
  return launch_status();
}

}  // extern "C"
