// Affine spatial transformer for gfx950, forward and backward: hdn_affine_sample_f32, hdn_affine_sample_bwd_f32.  The formulas are in
// include/hdn_hip.h.  Reference: ModelBuilder.stn_with_theta (model_builder_e2e_unconstrained_v2.py:233-237) = F.affine_grid + F.grid_sample with
// PyTorch's defaults (bilinear, padding_mode='zeros', align_corners=False); the grid [B,Ho,Wo,2] is never materialised here.
//
// One output pixel per lane, HDN_BLOCK lanes per workgroup, blockIdx.y = the sample; a lane walks the channels.  The call moves a few MB (B = 32:
// 25 MB of image, 6 MB of output) and is shaped by launch and gather latency, not by bandwidth: 256 consecutive output pixels (two output rows at
// Wo = 127) read four input rows' worth of taps, neighbouring lanes share cache lines, and 64 workgroups per sample (2048 at B = 32) keep every CU
// busy with eight waves per SIMD to hide the gathers.  Every tap address is clamped into the plane before it is formed and the loads are
// unconditional (the value is selected afterwards), so a lane issues its four loads back to back.
//
// sample_point() is the one place that turns (theta, pixel) into taps and weights: the forward and the backward both call it, so the backward
// differentiates through the taps the forward read.  A sample whose pixel position is not strictly inside (-1, W) x (-1, H) - NaN and values beyond
// any int included - is dead: the decision is a float comparison made before any conversion to an integer, its out is 0 and it contributes to no
// gradient (PyTorch's zeros padding gives 0 there too).
//
// grad_theta is deterministic: a lane adds its channels in ascending order (channels_bwd of geometry.h, the channel walk of every sampler backward),
// then block_sum_store of reduce.h (its fixed order; one partial of six floats per (sample, block) in the workspace) and reduce_partials_kernel of
// geometry.h (a second launch of the same call adds them in a fixed order).  64 partials per sample at 127 x 127: the second launch's one wave per sample reads each partial once.  grad_img is an fp32
// atomicAdd scatter into the buffer the call zero-fills on the stream, NOT bit-reproducible between calls.
#include "geometry.h"

#pragma clang fp contract(off)

namespace hdn {
namespace affine {

struct Point {
  float X, Y;                    // normalised output coordinate of the pixel, (2j+1)/Wo - 1 and (2i+1)/Ho - 1, rounded to fp32 (the chain factor of grad_theta)
  float w, e, n, s;              // w = px - floor(px), e = 1 - w, n = py - floor(py), s = 1 - n: each formed in float64 and rounded to fp32 once
  int i_nw, i_ne, i_sw, i_se;    // y * W + x of the four taps, clamped into the plane: always a valid index
  bool k_nw, k_ne, k_sw, k_se;   // does the tap lie inside [0,W) x [0,H) (and is the sample live)?  A tap that does not reads 0 and receives nothing
};

__device__ __forceinline__ Point sample_point(const float (&th)[6], int pix, int H, int W, int Ho, int Wo) {
  Point p;
  const int i = pix / Wo, j = pix - i * Wo;
  // the coordinate in float64 (contraction off: every operation rounded on its own, in the order written): a bilinear weight is px - floor(px), and an
  // fp32 px of size 100 would leave it 1e-5 of absolute error; this way the four weights' factors are float64 values rounded to fp32 once.  ~20 fp64 operations a lane.
  const double X = (double)(2 * j + 1) / (double)Wo - 1.0;
  const double Y = (double)(2 * i + 1) / (double)Ho - 1.0;
  const double gx = ((double)th[0] * X + (double)th[1] * Y) + (double)th[2];
  const double gy = ((double)th[3] * X + (double)th[4] * Y) + (double)th[5];
  const double px = ((gx + 1.0) * (double)W - 1.0) * 0.5;
  const double py = ((gy + 1.0) * (double)H - 1.0) * 0.5;
  // floating point first: NaN fails every comparison, +-inf and 1e30 fail one of them; only a live sample's floor is converted to an integer
  const bool live = px > -1.0 && px < (double)W && py > -1.0 && py < (double)H;
  const double xw = live ? floor(px) : 0.0, yn = live ? floor(py) : 0.0;
  p.X = (float)X;
  p.Y = (float)Y;
  const double dw = live ? px - xw : 0.0, dn = live ? py - yn : 0.0;
  p.w = (float)dw;
  p.n = (float)dn;
  p.e = (float)(1.0 - dw);  // not 1 - fp32(w): near w = 1 that difference would carry fp32(w)'s rounding at full size
  p.s = (float)(1.0 - dn);
  const int x0 = (int)xw, y0 = (int)yn;  // in [-1, W-1], [-1, H-1]
  const bool west = live && x0 >= 0, east = live && x0 + 1 < W, north = live && y0 >= 0, south = live && y0 + 1 < H;
  const int xa = clampi(x0, 0, W - 1), xb = clampi(x0 + 1, 0, W - 1), ya = clampi(y0, 0, H - 1), yb = clampi(y0 + 1, 0, H - 1);
  p.i_nw = ya * W + xa; p.i_ne = ya * W + xb; p.i_sw = yb * W + xa; p.i_se = yb * W + xb;
  p.k_nw = north && west; p.k_ne = north && east; p.k_sw = south && west; p.k_se = south && east;
  return p;
}

__device__ __forceinline__ void load_theta(const float* __restrict__ theta, int b, float (&th)[6]) {
#pragma unroll
  for (int q = 0; q < 6; ++q) th[q] = theta[size_t(b) * 6 + q];
}

__global__ __launch_bounds__(HDN_BLOCK) void sample_kernel(const float* __restrict__ img, const float* __restrict__ theta, float* __restrict__ out,
                                                           int C, int H, int W, int Ho, int Wo) {
  const int b = blockIdx.y;
  const int pix = blockIdx.x * HDN_BLOCK + threadIdx.x;
  if (pix >= Ho * Wo) return;
  float th[6];
  load_theta(theta, b, th);
  const Point p = sample_point(th, pix, H, W, Ho, Wo);
  const float nw = rn_mul(p.s, p.e), ne = rn_mul(p.s, p.w), sw = rn_mul(p.n, p.e), se = rn_mul(p.n, p.w);
  const size_t HW = size_t(H) * W, SS = size_t(Ho) * Wo;
  const float* im = img + size_t(b) * C * HW;
  float* o = out + size_t(b) * C * SS + pix;
  for (int c = 0; c < C; ++c) {
    const float* pl = im + c * HW;
    const float l_nw = pl[p.i_nw], l_ne = pl[p.i_ne], l_sw = pl[p.i_sw], l_se = pl[p.i_se];
    const float v_nw = p.k_nw ? l_nw : 0.f, v_ne = p.k_ne ? l_ne : 0.f, v_sw = p.k_sw ? l_sw : 0.f, v_se = p.k_se ? l_se : 0.f;
    o[size_t(c) * SS] = rn_add(rn_add(rn_add(rn_mul(v_nw, nw), rn_mul(v_ne, ne)), rn_mul(v_sw, sw)), rn_mul(v_se, se));
  }
}

__global__ __launch_bounds__(HDN_BLOCK) void sample_bwd_kernel(const float* __restrict__ img, const float* __restrict__ theta,
                                                               const float* __restrict__ gout, float* __restrict__ part, float* __restrict__ gimg,
                                                               int C, int H, int W, int Ho, int Wo) {
  __shared__ float red[BLOCK_WAVES * 6];
  const int b = blockIdx.y;
  const int pix = blockIdx.x * HDN_BLOCK + threadIdx.x;
  float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (pix < Ho * Wo) {
    float th[6];
    load_theta(theta, b, th);
    const Point p = sample_point(th, pix, H, W, Ho, Wo);
    const gbwd::Taps t = {p.i_nw, p.i_ne, p.i_sw, p.i_se, p.k_nw, p.k_ne, p.k_sw, p.k_se, p.e, p.w, p.s, p.n};
    const size_t HW = size_t(H) * W, SS = size_t(Ho) * Wo;
    float ax = 0.f, ay = 0.f;  // sum over channels of gout * d out / d px, d out / d py
    gbwd::channels_bwd(t, img + size_t(b) * C * HW, gimg ? gimg + size_t(b) * C * HW : nullptr, HW, gout + size_t(b) * C * SS + pix, SS, C,
                       part != nullptr, ax, ay);
    // d px / d gx = W/2, d py / d gy = H/2;  g_r = theta[r,0] X + theta[r,1] Y + theta[r,2]
    ax = rn_mul(ax, rn_mul((float)W, 0.5f));
    ay = rn_mul(ay, rn_mul((float)H, 0.5f));
    acc[0] = rn_mul(ax, p.X); acc[1] = rn_mul(ax, p.Y); acc[2] = ax;
    acc[3] = rn_mul(ay, p.X); acc[4] = rn_mul(ay, p.Y); acc[5] = ay;
  }
  if (part) block_sum_store<6, BLOCK_WAVES>(acc, red, part + (size_t(b) * gridDim.x + blockIdx.x) * 6);  // kernel-uniform branch
}

static int check_dims(int B, int C, int H, int W, int Ho, int Wo) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0) return HDN_E_SHAPE;
  return HDN_OK;
}

static bool over_limit(int B, long long in_px, long long out_px) { return B > 65535 || in_px > (1LL << 30) || out_px > (1LL << 30); }

}  // namespace affine
}  // namespace hdn

extern "C" {

int hdn_affine_sample_f32(const float* img, const float* theta, float* out, int B, int C, int H, int W, int Ho, int Wo, void* stream) {
  using namespace hdn;
  if (!img || !theta || !out) return HDN_E_NULL;
  if (affine::check_dims(B, C, H, W, Ho, Wo)) return HDN_E_SHAPE;
  if (affine::over_limit(B, (long long)H * W, (long long)Ho * Wo)) return HDN_E_LIMIT;
  if (out == img || out == theta) return HDN_E_ALIAS;
  hipLaunchKernelGGL(affine::sample_kernel, dim3(cdiv(Ho * Wo, HDN_BLOCK), B), dim3(HDN_BLOCK), 0, static_cast<hipStream_t>(stream), img, theta, out,
                     C, H, W, Ho, Wo);
  return launch_status();
}

long long hdn_affine_sample_bwd_workspace_bytes(int B, int Ho, int Wo) {
  if (B <= 0 || Ho <= 0 || Wo <= 0) return HDN_E_SHAPE;
  if (B > 65535 || (long long)Ho * Wo > (1LL << 30)) return HDN_E_LIMIT;
  return (long long)B * hdn::cdiv(Ho * Wo, HDN_BLOCK) * 6 * sizeof(float);
}

int hdn_affine_sample_bwd_f32(const float* img, const float* theta, const float* grad_out, float* grad_theta_or_null, float* grad_img_or_null,
                              float* workspace, long long workspace_bytes, int B, int C, int H, int W, int Ho, int Wo, void* stream) {
  using namespace hdn;
  if (!img || !theta || !grad_out) return HDN_E_NULL;
  if (affine::check_dims(B, C, H, W, Ho, Wo) || (!grad_theta_or_null && !grad_img_or_null)) return HDN_E_SHAPE;
  if (affine::over_limit(B, (long long)H * W, (long long)Ho * Wo)) return HDN_E_LIMIT;
  const long long img_floats = (long long)B * C * H * W, out_floats = (long long)B * C * Ho * Wo;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int nblk = cdiv(Ho * Wo, HDN_BLOCK);
  return gbwd::sampler_bwd<6>({img, theta, grad_out}, img_floats, out_floats, grad_theta_or_null, grad_img_or_null, workspace, workspace_bytes,
                              hdn_affine_sample_bwd_workspace_bytes(B, Ho, Wo), nblk, B, 1.0f, 1.0f, st, [&](float* part) {
                                hipLaunchKernelGGL(affine::sample_bwd_kernel, dim3(nblk, B), dim3(HDN_BLOCK), 0, st, img, theta, grad_out, part,
                                                   grad_img_or_null, C, H, W, Ho, Wo);
                              });
}

}  // extern "C"
