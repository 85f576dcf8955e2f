// conv1x1.hip — the 1x1 convolutions of the ResNet-50 (Bottleneck) homography trunk, bias / residual / ReLU fused, on the matrix cores.
//
//   out[B,So,So,CO] = epilogue( x[B,S,S,CI] sampled at stride s  .  W^T ),   So = (S - 1) / s + 1, channels-last in and out
//   epilogue: + bias[co] (+ residual[B,So,So,CO]) (ReLU)
//
// Replaces conv1 + bn1 + relu, conv3 + bn3 (+ residual) + relu and the downsample branch (Conv2d(CI, CO, 1, s) + BatchNorm2d) of
// homo_estimator/Deep_homography/Oneline_DLTv1/backbone/resnet.py:97-133, 162-176 (eval mode, BatchNorm folded by the caller).
//
// An implicit GEMM, M = B So^2 pixels, N = CO, K = CI, with fp32 carried as two fp16 pieces on v_mfma_f32_32x32x16_f16 (mfma_split.h: three
// piece products into "hi" / "lo" fp32 accumulators, the error of an fp32 product; activations split as x 2^-8, or already stored so with act_domain = 1).
// D = A . B with A = activations (row = pixel, one lane per (pixel, k half)) and B = packed weights (column = output channel): a lane's accumulator
// column is ONE output channel, so its bias is one register and every store of a register is 32 consecutive channels of a pixel (128 bytes per half-wave).
// K walks in chunks of 32 input channels; inside a chunk lane (pixel, g) reads the 16 consecutive channels [16 g, 16 g + 16) of its pixel (64 bytes,
// four 16-byte loads; the two half-waves together read a whole 128-byte line per pixel) and feeds channels 16 g + 8 t + [0, 8) to k step t — the packer
// (csrc/pack.hip, hdn_pack_conv1x1_f32) lays the weights out in that k order.  Activations go global -> registers (no LDS image: each is used by
// the 32 NT output channels of the wave that loads it); weights stream L2 -> registers in fragment order, 16 bytes per lane.  The next chunk's loads
// are issued before the current chunk's MFMAs.
//
// Workgroup = 4 waves = WM pixel tiles x WN output-channel groups x KW slices of K; a wave owns 32 pixels x 32 NT channels.  Large problems use
// KW = 1 (no reduction); when they give fewer than FILL workgroups (the tracker's B = 1: M = 16 at layer 4) and K allows it, the small-M form
// (NT = 1, KW = 4) splits K over the four waves of a workgroup and adds the partial sums through the LDS in a fixed order (deterministic).
#include <climits>

#include "hdn_common.h"
#include "mfma_split.h"

namespace hdn {
namespace c1 {
using namespace hdn::mc;

constexpr int FILL = 512;       // workgroups below which the small-M form is used (2 per CU)

template <int NT_, int WM_, int WN_, int KW_>
struct Cfg {
  static constexpr int NT = NT_, WM = WM_, WN = WN_, KW = KW_;
  static_assert(WM * WN * KW == 4, "four waves per workgroup");
};

template <class C, bool SD>
__global__ __launch_bounds__(256) void conv1x1_kernel(const float* __restrict__ x, const u32x4* __restrict__ wp, const float* __restrict__ bias,
                                                      const float* __restrict__ res, float* __restrict__ out, int M, int So, int S, int stride, int CI,
                                                      int CO, int relu) {
  constexpr int NT = C::NT, WN = C::WN, KW = C::KW;
  __shared__ float red[KW > 1 ? C::WM * WN * (KW - 1) * NT * 16 * 64 : 1];     // [wave of the slice group - 1][n tile][register][lane]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wk = wave % KW, wn = (wave / KW) % WN, wm = wave / (KW * WN);
  const int li = lane & 31, g = lane >> 5;
  const int m0 = (blockIdx.x * C::WM + wm) * 32;
  const int nt0 = (blockIdx.y * WN + wn) * NT;                              // the wave's first 32-channel output tile

  // this lane's A row: pixel m0 + li (clamped to the last pixel: loaded, never stored)
  const int m = min(m0 + li, M - 1), so2 = So * So;
  const int b = m / so2, rm = m - b * so2, oy = rm / So, ox = rm - oy * So;
  const float* xr = x + (((size_t)b * S + (size_t)oy * stride) * S + (size_t)ox * stride) * CI + 16 * g;
  const int chunks = CI >> 5, cpk = chunks / KW, c0 = wk * cpk;
  const size_t wtile = (size_t)chunks * 4 * 64;                             // u32x4 per 32-channel output tile: [chunk][k step][piece][lane]
  const u32x4* wl = wp + (size_t)nt0 * wtile + (size_t)c0 * 4 * 64 + lane;

  f32x16 hi[NT], lo[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) hi[j][r] = lo[j][r] = 0.f;

  f4 xa[4];
  u32x4 wa[NT][4];
  auto load = [&](int c) {
    const f4* xs = reinterpret_cast<const f4*>(xr + (size_t)(c0 + c) * 32);
#pragma unroll
    for (int q = 0; q < 4; ++q) xa[q] = xs[q];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) wa[j][q] = wl[(size_t)j * wtile + ((size_t)c * 4 + q) * 64];
  };
  load(0);
  for (int c = 0; c < cpk; ++c) {
    f4 xv[4];
    u32x4 wv[NT][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) xv[q] = xa[q];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) wv[j][q] = wa[j][q];
    if (c + 1 < cpk) load(c + 1);
    mma_chunk<SD>(xv, wv, hi, lo);
  }

  // joined partial sums; with K split over the waves, the slices 1 .. KW - 1 hand theirs to slice 0 through the LDS
  float p[NT][16];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) p[j][r] = join<SD>(hi[j][r], lo[j][r]);
  if constexpr (KW > 1) {
    const int grp = wm * WN + wn;
    if (wk > 0) {
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) red[(((grp * (KW - 1) + wk - 1) * NT + j) * 16 + r) * 64 + lane] = p[j][r];
    }
    __syncthreads();
    if (wk > 0) return;
#pragma unroll
    for (int s = 0; s < KW - 1; ++s)
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) p[j][r] += red[(((grp * (KW - 1) + s) * NT + j) * 16 + r) * 64 + lane];
  }

  // epilogue: register r of a lane is pixel m0 + d_row(r, g), output channel 32 (nt0 + j) + li
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int co = (nt0 + j) * 32 + li;
    const float bv = bias[co];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int mm = m0 + d_row(r, g);
      if (mm < M) {
        const size_t o = (size_t)mm * CO + co;
        float v = p[j][r] + bv;
        if (res) v += res[o];
        if (relu) v = fmaxf(v, 0.f);
        out[o] = v;
      }
    }
  }
}

template <class C, bool SD>
static int launch(const float* x, const void* wp, const float* bias, const float* res, float* out, int B, int S, int CI, int CO, int stride, int relu,
                  hipStream_t s) {
  const int So = (S - 1) / stride + 1;
  const int M = B * So * So;
  const dim3 grid((unsigned)cdiv(M, 32 * C::WM), (unsigned)(CO / (32 * C::NT * C::WN)));
  hipLaunchKernelGGL((conv1x1_kernel<C, SD>), grid, dim3(256), 0, s, x, static_cast<const u32x4*>(wp), bias, res, out, M, So, S, stride, CI, CO, relu);
  return launch_status();
}

// the schedule for a problem: f(Cfg<...>{}) with the form chosen as described at the top
template <class F>
static int dispatch(int M, int CI, int CO, F&& f) {
  if (CO % 64) return f(Cfg<1, 4, 1, 1>{});
  const int n64 = CO / 64, chunks = CI / 32;
  const int wn = n64 % 4 == 0 ? 4 : n64 % 2 == 0 ? 2 : 1;
  const long long wgs = (long long)cdiv(M, 32 * (4 / wn)) * (n64 / wn);
  if (wgs < FILL && chunks % 4 == 0) return f(Cfg<1, 1, 1, 4>{});
  if (wn == 4) return f(Cfg<2, 1, 4, 1>{});
  if (wn == 2) return f(Cfg<2, 2, 2, 1>{});
  return f(Cfg<2, 4, 1, 1>{});
}

}  // namespace c1
}  // namespace hdn

// the launch form dispatch() picks for a problem, for tests and profiles: NT | WM << 8 | WN << 16 | KW << 24.  Host only: nothing is launched.
extern "C" int hdn_conv1x1_form(int B, int S, int CI, int CO, int stride) {
  if (B <= 0 || S <= 0 || CI <= 0 || CO <= 0 || CI % 32 || CO % 32 || (stride != 1 && stride != 2)) return HDN_E_SHAPE;
  const long long So = (S - 1) / stride + 1;
  const long long nx = (long long)B * S * S * CI, nout = (long long)B * So * So * CO;
  if (nx > INT_MAX || nout > INT_MAX || CO > 65536) return HDN_E_LIMIT;
  return hdn::c1::dispatch((int)(B * So * So), CI, CO, [](auto cfg) {
    using C = decltype(cfg);
    return C::NT | C::WM << 8 | C::WN << 16 | C::KW << 24;
  });
}

extern "C" int hdn_conv1x1_f32(const float* x, const void* wpacked, const float* bias, const float* residual, float* out, int B, int S, int CI, int CO,
                               int stride, int relu, int act_domain, void* stream) {
  if (!x || !wpacked || !bias || !out) return HDN_E_NULL;
  if (B <= 0 || S <= 0 || CI <= 0 || CO <= 0 || CI % 32 || CO % 32 || (stride != 1 && stride != 2) || (relu != 0 && relu != 1) ||
      (act_domain != 0 && act_domain != 1))
    return HDN_E_SHAPE;
  const long long So = (S - 1) / stride + 1;
  const long long nx = (long long)B * S * S * CI, nout = (long long)B * So * So * CO;
  if (nx > INT_MAX || nout > INT_MAX || CO > 65536) return HDN_E_LIMIT;
  if (hdn::bytes_overlap(out, nout * 4, x, nx * 4) || (residual && hdn::bytes_overlap(out, nout * 4, residual, nout * 4))) return HDN_E_ALIAS;
  if (!hdn::aligned16(x) || !hdn::aligned16(wpacked) || !hdn::aligned16(out) || (residual && !hdn::aligned16(residual))) return HDN_E_LIMIT;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (const int rr = hdn::check_fp16_range(x, nx, s, act_domain)) return rr;
  return hdn::c1::dispatch((int)(B * So * So), CI, CO, [&](auto cfg) {
    return hdn::mc::by_domain(act_domain, [&](auto sd) {
      return hdn::c1::launch<decltype(cfg), decltype(sd)::value>(x, wpacked, bias, residual, out, B, S, CI, CO, stride, relu, s);
    });
  });
}
