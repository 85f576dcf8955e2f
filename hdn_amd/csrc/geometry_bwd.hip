// Backward of the three geometry operators for gfx950 (training only): hdn_logpolar_sample_bwd_f32 (logpolar.hip), hdn_dlt_solve_bwd_f32 and
// hdn_warp_bwd_f32 (dlt_warp.hip).  The formulas are in include/hdn_hip.h.
//
// Each kernel recomputes its forward's sample point by calling the function the forward calls (logpolar_point, warp_point, dlt_row + solve8 of
// geometry.h), so the taps it differentiates through are the taps the forward read; the channel walk of the two samplers is channels_bwd
// (geometry.h), shared with affine_stn.hip, and the entry points' host sequence is sampler_bwd.  The launch shapes are the forward's: HDN_BLOCK
// threads, one pixel per lane in the sampler, WARP_PX_PER_THREAD per thread in the warp, one 8-lane group per sample in the solve.
//
// grad_polar / grad_theta (a sum over every pixel and channel of a sample) are deterministic and use no atomics: a lane adds its channels (and, in
// the warp, its pixels) in ascending order, the block adds them in the fixed order of reduce.h (block_sum_store) and writes one partial per
// (sample, block) into the caller's workspace; reduce_partials_kernel (geometry.h), a second launch of the same call, has one wave per sample
// add the partials (lane l takes blocks l, l + 64, ... in ascending order, then wave_sum).  Nothing depends on the batch size:
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
  __shared__ float red[BLOCK_WAVES * 2];
  const int n = blockIdx.y;
  const int pix = blockIdx.x * HDN_BLOCK + threadIdx.x;
  float acc[2] = {0.f, 0.f};  // sum over channels of gout * d out / d px, d out / d py, times the border rule
  if (pix < S * S) {
    const LogpolarPoint p = logpolar_point(polar, rho, cosT, sinT, n, pix, H, W, S);
    // clip_coordinates_set_grad: a coordinate that the clamp moved (or that sits on the border) has derivative 0
    const float mx = (p.pxu <= 0.0f || p.pxu >= (float)(W - 1)) ? 0.f : 1.f;
    const float my = (p.pyu <= 0.0f || p.pyu >= (float)(H - 1)) ? 0.f : 1.f;
    const Taps t = {p.y0 * W + p.x0, p.y0 * W + p.x1, p.y1 * W + p.x0, p.y1 * W + p.x1, true, p.e_ok, p.s_ok, p.e_ok && p.s_ok, p.e, p.w, p.s, p.nn};
    const size_t HW = size_t(H) * W, SS = size_t(S) * S;
    channels_bwd(t, img + size_t(n) * C * HW, gimg ? gimg + size_t(n) * C * HW : nullptr, HW, gout + size_t(n) * C * SS + pix, SS, C, part != nullptr,
                 acc[0], acc[1]);
    acc[0] = rn_mul(acc[0], mx);
    acc[1] = rn_mul(acc[1], my);
  }
  if (part) block_sum_store<2, BLOCK_WAVES>(acc, red, part + (size_t(n) * gridDim.x + blockIdx.x) * 2);  // kernel-uniform branch
}

// ---------------------------------------------------------------------------------------------------------------- DLT solve
__global__ __launch_bounds__(HDN_BLOCK) void dlt_solve_bwd_kernel(const float* __restrict__ src, const float* __restrict__ off,
                                                                  const float* __restrict__ gH, float* __restrict__ gsrc,
                                                                  float* __restrict__ goff, int B) {
  const int gid = (blockIdx.x * HDN_BLOCK + threadIdx.x) >> 3;
  const int b = min(gid, B - 1);  // keep every lane in the shuffles
  const int r = threadIdx.x & 7;
  const float* s = src + size_t(b) * 8;
  const float* o = off + size_t(b) * 8;
  const double h = solve8(dlt_row(s, o, r), r);  // A h = b, the forward's own solve
  Row9 at;
#pragma unroll
  for (int j = 0; j < 8; ++j) at.v[j] = dlt_elem(s, o, j, r);  // row r of A^T
  at.v[8] = (double)gH[size_t(b) * 9 + r];                     // gH[8] meets the constant 1
  const double lam = solve8(at, r);  // A^T lambda = grad_h;  grad_b = lambda, grad_A = -lambda h^T
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
  __shared__ float red[BLOCK_WAVES * 9];
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
    const WarpPoint p = warp_point(th, i, j, H, W);
    // the integer taps are constants; the nudge has derivative 1.  Taps a, b, c, d of the forward are nw, sw, ne, se; its weights wa .. wd are
    // ax ay, ax by, bx ay, bx by, so (ax, bx, ay, by) stand where a sampler has (e, w, s, n).  Every tap is clamped into the plane and kept.
    const Taps t = {p.y0 * W + p.x0, p.y0 * W + p.x1, p.y1 * W + p.x0, p.y1 * W + p.x1, true, true, true, true, p.ax, p.bx, p.ay, p.by};
    float sx = 0.f, sy = 0.f;  // sum over channels of gout * d out / d x, d out / d y
    channels_bwd(t, im, gi, HW, gb + size_t(pix) * C, 1, C, part != nullptr, sx, sy);
    if (part) {
      // x = (xs + 1) W / 2, xs = T0 / t:  d x / d T0 = (W/2) / t,  d x / d t = -(W/2) xs / t
      const float gxs = rn_mul(sx, rn_mul((float)W, 0.5f)), gys = rn_mul(sy, rn_mul((float)H, 0.5f));
      const float g0 = rn_div(gxs, p.t), g1 = rn_div(gys, p.t);
      const float g2 = -rn_div(rn_add(rn_mul(gxs, p.xs), rn_mul(gys, p.ys)), p.t);
      // T_r = theta[3r] gx + theta[3r+1] gy + theta[3r+2]
      acc[0] = rn_add(acc[0], rn_mul(g0, p.gx)); acc[1] = rn_add(acc[1], rn_mul(g0, p.gy)); acc[2] = rn_add(acc[2], g0);
      acc[3] = rn_add(acc[3], rn_mul(g1, p.gx)); acc[4] = rn_add(acc[4], rn_mul(g1, p.gy)); acc[5] = rn_add(acc[5], g1);
      acc[6] = rn_add(acc[6], rn_mul(g2, p.gx)); acc[7] = rn_add(acc[7], rn_mul(g2, p.gy)); acc[8] = rn_add(acc[8], g2);
    }
  }
  if (part) block_sum_store<9, BLOCK_WAVES>(acc, red, part + (size_t(b) * gridDim.x + blockIdx.x) * 9);  // kernel-uniform branch
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
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int nblk = cdiv(S * S, HDN_BLOCK);
  // d px / d polar_x = (W/2) / (H//2), d py / d polar_y = (H/2) / (W//2): the forward's (sic) pairing
  const float fx = (float)W * 0.5f / (float)(H / 2), fy = (float)H * 0.5f / (float)(W / 2);
  return gbwd::sampler_bwd<2>({img, polar, rho, cos_theta, sin_theta, grad_out}, img_floats, out_floats, grad_polar_or_null, grad_img_or_null,
                              workspace, workspace_bytes, hdn_logpolar_sample_bwd_workspace_bytes(B, S), nblk, B, fx, fy, st, [&](float* part) {
                                hipLaunchKernelGGL(gbwd::logpolar_bwd_kernel, dim3(nblk, B), dim3(HDN_BLOCK), 0, st, img, polar, rho, cos_theta,
                                                   sin_theta, grad_out, part, grad_img_or_null, C, H, W, S);
                              });
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
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int nblk = cdiv(H * W, WARP_PX_PER_BLOCK);
  return gbwd::sampler_bwd<9>({img, theta, grad_out}, img_floats, img_floats, grad_theta_or_null, grad_img_or_null, workspace, workspace_bytes,
                              hdn_warp_bwd_workspace_bytes(B, H, W), nblk, B, 1.0f, 1.0f, st, [&](float* part) {
                                hipLaunchKernelGGL(gbwd::warp_bwd_kernel, dim3(nblk, B), dim3(HDN_BLOCK), 0, st, img, theta, grad_out, part,
                                                   grad_img_or_null, C, H, W);
                              });
}

}  // extern "C"
