// conv3x3d.hip — the dilated 3x3 convolutions of the similarity branch's ResNet-50 (stride 8, atrous), bias / ReLU fused, on the matrix cores.
//
//   out[B,S,S,CO] = epilogue( conv3x3(x[B,S,S,CI]; stride 1, dilation d, zero padding d) ),   channels-last fp32 in and out, d = 1 / 2 / 4
//   epilogue: (+ bias[co]) (ReLU)
//
// Replaces conv2 + bn2 + relu of a Bottleneck and the 3x3 downsample branches (Conv2d(CI, CO, 3, padding = dilation) + BatchNorm2d) of
// hdn/models/backbone/resnet_atrous.py:62-110, 152-183 (eval mode, BatchNorm folded by the caller).
//
// conv1x1.hip's implicit GEMM run over nine taps: M = B S^2 pixels, N = CO, K = 9 CI, fp32 carried as two fp16 pieces on v_mfma_f32_32x32x16_f16
// (mfma_split.h: three piece products into "hi" / "lo" accumulators).  D = A . B with A = activations (row = pixel, one lane per (pixel, k half)) and
// B = packed weights (column = output channel): a lane's accumulator column is ONE output channel.  K walks in STEPS of one tap x 32 input channels,
// tap-major (step = tap * CI / 32 + chunk, tap = 3 ky + kx); in a step lane (pixel, g) reads the 16 channels [16 g, 16 g + 16) of the pixel at
// ((ky - 1) d, (kx - 1) d) from its own — under a predicate: a tap that leaves the image loads nothing and contributes zeros (S <= d: only the centre
// tap is ever in bounds) — and feeds channels 16 g + 8 t + [0, 8) to k step t; the packer (csrc/pack.hip, hdn_pack_conv3x3d_f32) lays the weights out
// in that order, so they stream L2 -> registers in fragment order, 16 bytes per lane.  The next step's loads are issued before the current step's MFMAs.
//
// Workgroup = 4 waves = WM x WN waves of MT x NT 32 x 32 tiles each; every form covers 128 pixels, so at M = 961 (B = 1, side 31) the weights are
// read 8 times, not 31.  The weight stream is the big operand (1024 -> 2048: 75 MB): the grid is one-dimensional with the PIXEL tile running fastest —
// workgroups that share a weight tile are neighbours — and remapped so that neighbours share an XCD (and with it an L2) instead of being dealt out
// round-robin over the eight.  Forms (dispatch()):
//   A  Cfg<1, 1, 4, 1>   128 pixels x  32 channels   CO not a multiple of 64
//   B  Cfg<1, 2, 4, 1>   128 pixels x  64 channels   problems that would not give form C one workgroup per CU
//   C  Cfg<2, 2, 2, 2>   128 pixels x 128 channels   CO a multiple of 128 and at least FILL such workgroups (64 x 64 per wave: half the loads per MFMA)
// A and B with fewer than FILL workgroups (the tracker's B = 1) split K over grid.y into Z slices of whole steps; every slice writes its joined partial
// tile to `workspace` [z][M][CO] and finish_slices (epilogue.hip) adds the slices in slice order with the bias and the ReLU: deterministic, no atomics.
//
// hdn_conv3x3v_f32 (further down) is the same kernel with another pixel map (template parameter VALID): padding 0, stride s = 1 / 2,
//   out[B,So,So,CO] = epilogue( conv3x3(x[B,S,S,CI]; stride s, dilation 1, no padding) ),   So = (S - 3) / s + 1,   M = B So^2
// — conv2 and the 3x3 skip of layer2's first block (resnet_atrous.py:70-81 `padding = 2 - stride`, :162-174).  Output pixel (oy, ox) reads input pixel
// (s oy + ky, s ox + kx): no tap ever leaves the image, so the predicate drops out; weights, K order, forms, K split and finish pass are the ones above.
#include <climits>

#include "hdn_common.h"
#include "mfma_split.h"

namespace hdn {
namespace c3d {
using namespace hdn::mc;

constexpr int FILL = 256;       // workgroups below which K is split (one per CU)
constexpr int MAX_Z = 16;       // most K slices
constexpr int MIN_STEPS = 4;    // fewest K steps worth a slice
constexpr int NXCD = 8;

template <int MT_, int NT_, int WM_, int WN_>
struct Cfg {
  static constexpr int MT = MT_, NT = NT_, WM = WM_, WN = WN_;
  static constexpr int BM = 32 * MT * WM, BN = 32 * NT * WN;
  static_assert(WM * WN == 4, "four waves per workgroup");
};

// FINAL: the whole of K in this workgroup, epilogue here; otherwise slice blockIdx.y of K, raw joined sums to dst = workspace [z][M][CO]
// VALID: the padding-0 pixel map — M = B So^2 output pixels, `d` is the STRIDE, a tap is never out of bounds; otherwise So == S and `d` is the dilation
// MAP: the pixel map — SAME (padding = dilation), VALID (above) or FULL (padding 2, stride 1: So = S + 2 outputs per side, the tap (ky, kx) of output
//   pixel (oy, ox) reads input pixel (oy + ky - 2, ox + kx - 2) under the out-of-image predicate: the input gradient of a valid convolution, see
//   hdn_conv3x3v_dgrad_f32 further down).
// GRAD: x is a GRADIENT — split as x 2^ge (ge: the exponent hdn_grad_scale_f32 chose from the data, conv3x3_train.hip) instead of the activations'
//   fixed 2^-8, the join multiplies by 2^-ge; no bias, no ReLU.
enum PixelMap { SAME = 0, VALID_MAP = 1, FULL = 2 };

template <class C, bool SD, bool FINAL, int MAP, bool GRAD>
__device__ __forceinline__ void conv3x3d_body(const float* __restrict__ x, const u32x4* __restrict__ wp, const float* __restrict__ bias,
                                              float* __restrict__ dst, int M, int S, int So, int d, int CI, int CO, int relu, int tm, int sps, int ge) {
  constexpr bool VALID = MAP == VALID_MAP;
  constexpr int MT = C::MT, NT = C::NT, WN = C::WN;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn = wave % WN, wm = wave / WN;
  const int li = lane & 31, g = lane >> 5;
  // consecutive workgroup ids go to consecutive XCDs: give every XCD a contiguous run of tiles instead (bijective for any grid size)
  const int nwg = gridDim.x, orig = blockIdx.x, xcd = orig % NXCD, q = nwg / NXCD, r = nwg % NXCD;
  const int id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + orig / NXCD;
  const int pm = id % tm, pn = id / tm;                                     // pixel tile fastest: neighbours share the weight tile
  const int m0 = (pm * C::WM + wm) * (32 * MT);
  const int nt0 = (pn * WN + wn) * NT;                                      // the wave's first 32-channel output tile

  // this lane's A rows: pixels m0 + 32 i + li (clamped to the last pixel: loaded, never stored)
  const float* xr[MT];
  int oy[MT], ox[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int m = min(m0 + 32 * i + li, M - 1), s2 = So * So;
    const int b = m / s2, rm = m - b * s2;
    oy[i] = rm / So;
    ox[i] = rm - oy[i] * So;
    if constexpr (VALID) xr[i] = x + (((size_t)b * S + d * oy[i]) * S + d * ox[i]) * CI + 16 * g;      // the window's top-left pixel
    else if constexpr (MAP == FULL) xr[i] = x + (((ptrdiff_t)b * S + oy[i]) * S + ox[i]) * CI + 16 * g;   // input pixel (oy, ox): read only at in-image taps
    else xr[i] = x + (size_t)m * CI + 16 * g;
  }
  const int chunks = CI >> 5, steps = 9 * chunks;
  const int s0 = FINAL ? 0 : (int)blockIdx.y * sps, s1 = FINAL ? steps : min(steps, s0 + sps);
  const size_t wtile = (size_t)steps * 4 * 64;                              // u32x4 per 32-channel output tile: [tap][chunk][k step][piece][lane]
  const u32x4* wl = wp + (size_t)nt0 * wtile + lane;

  f32x16 hi[MT][NT], lo[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int rr = 0; rr < 16; ++rr) hi[i][j][rr] = lo[i][j][rr] = 0.f;

  f4 xa[MT][4];
  u32x4 wa[NT][4];
  int tap = s0 / chunks, c = s0 - tap * chunks;                             // of the next step to load
  auto load = [&](int s) {
    const int ky = tap / 3, kx = tap - 3 * ky;
    const int dy = VALID ? ky : MAP == FULL ? ky - 2 : (ky - 1) * d, dx = VALID ? kx : MAP == FULL ? kx - 2 : (kx - 1) * d;
    const ptrdiff_t off = ((ptrdiff_t)dy * S + dx) * CI + c * 32;
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const bool in = VALID || ((unsigned)(oy[i] + dy) < (unsigned)S && (unsigned)(ox[i] + dx) < (unsigned)S);
      const f4* xs = reinterpret_cast<const f4*>(xr[i] + off);
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) xa[i][qq] = in ? xs[qq] : f4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) wa[j][qq] = wl[(size_t)j * wtile + ((size_t)s * 4 + qq) * 64];
    if (++c == chunks) { c = 0; ++tap; }
  };
  load(s0);
  for (int s = s0; s < s1; ++s) {
    f4 xv[MT][4];
    u32x4 wv[NT][4];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) {
        xv[i][qq] = xa[i][qq];
        if constexpr (GRAD) xv[i][qq] = f4{ldexpf(xv[i][qq].x, ge), ldexpf(xv[i][qq].y, ge), ldexpf(xv[i][qq].z, ge), ldexpf(xv[i][qq].w, ge)};
      }
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) wv[j][qq] = wa[j][qq];
    if (s + 1 < s1) load(s + 1);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < MT; ++i) mma_kstep<SD || GRAD>(t, xv[i], wv, hi[i], lo[i]);
  }

  // epilogue: register r of a lane is pixel m0 + 32 i + d_row(r, g), output channel 32 (nt0 + j) + li
  float* o = FINAL ? dst : dst + (size_t)blockIdx.y * M * CO;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int co = (nt0 + j) * 32 + li;
    const float bv = (FINAL && bias) ? bias[co] : 0.f;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int rr = 0; rr < 16; ++rr) {
        const int mm = m0 + 32 * i + d_row(rr, g);
        if (mm < M) {
          float v = join<SD || GRAD>(hi[i][j][rr], lo[i][j][rr]);
          if constexpr (GRAD) v = ldexpf(v, -ge);
          if (FINAL && !GRAD) {
            v += bv;
            if (relu) v = fmaxf(v, 0.f);
          }
          o[(size_t)mm * CO + co] = v;
        }
      }
  }
}

template <class C, bool SD, bool FINAL, bool VALID = false>
__global__ __launch_bounds__(256) void conv3x3d_kernel(const float* __restrict__ x, const u32x4* __restrict__ wp, const float* __restrict__ bias,
                                                       float* __restrict__ dst, int M, int S, int So, int d, int CI, int CO, int relu, int tm, int sps) {
  conv3x3d_body<C, SD, FINAL, VALID ? VALID_MAP : SAME, false>(x, wp, bias, dst, M, S, So, d, CI, CO, relu, tm, sps, 0);
}

// the input gradient of the valid stride-1 convolution: x = dy [B, S, S, CI = the convolution's CO], So = S + 2, *expp = the split exponent
template <class C, bool FINAL>
__global__ __launch_bounds__(256) void conv3x3_dgrad_kernel(const float* __restrict__ x, const u32x4* __restrict__ wp, const int* __restrict__ expp,
                                                            float* __restrict__ dst, int M, int S, int So, int CI, int CO, int tm, int sps) {
  conv3x3d_body<C, false, FINAL, FULL, true>(x, wp, nullptr, dst, M, S, So, 1, CI, CO, 0, tm, sps, *expp);
}

// K steps per slice for a form that gives `wgs` workgroups over `steps` K steps (steps: one slice, no workspace)
static int steps_per_slice(long long wgs, int steps) {
  if (wgs >= FILL) return steps;
  long long z = (FILL + wgs - 1) / wgs;
  if (z > MAX_Z) z = MAX_Z;
  if (z > steps / MIN_STEPS) z = steps / MIN_STEPS;
  if (z < 1) z = 1;
  return (steps + (int)z - 1) / (int)z;
}

// the schedule for a problem: f(Cfg<...>{}, K steps per slice) with the form chosen as described at the top
template <class F>
static long long dispatch(long long M, int CI, int CO, F&& f) {
  const int steps = 9 * (CI / 32);
  const long long tm = (M + 127) / 128;
  if (CO % 64) return f(Cfg<1, 1, 4, 1>{}, steps_per_slice(tm * (CO / 32), steps));
  if (CO % 128 == 0 && tm * (CO / 128) >= FILL) return f(Cfg<2, 2, 2, 2>{}, steps);
  return f(Cfg<1, 2, 4, 1>{}, steps_per_slice(tm * (CO / 64), steps));
}

template <class C, bool SD, bool VALID = false>
static int launch(const float* x, const void* wp, const float* bias, float* out, float* ws, int M, int S, int So, int d, int CI, int CO, int relu, int sps,
                  hipStream_t s) {
  const int steps = 9 * (CI / 32), Z = cdiv(steps, sps), tm = cdiv(M, C::BM);
  const dim3 grid((unsigned)((long long)tm * (CO / C::BN)), (unsigned)Z);
  const u32x4* w = static_cast<const u32x4*>(wp);
  if (Z == 1) {
    hipLaunchKernelGGL((conv3x3d_kernel<C, SD, true, VALID>), grid, dim3(256), 0, s, x, w, bias, out, M, S, So, d, CI, CO, relu, tm, sps);
    return launch_status();
  }
  hipLaunchKernelGGL((conv3x3d_kernel<C, SD, false, VALID>), grid, dim3(256), 0, s, x, w, bias, ws, M, S, So, d, CI, CO, relu, tm, sps);
  if (const int rc = launch_status()) return rc;
  return finish_slices(ws, Z, bias, relu, out, (long long)M * CO, CO, s);
}

// HDN_OK, or what the entry points answer for a shape they do not take.  step: the dilation (1 / 2 / 4: stride 1, padding = dilation) or, VALID, the stride
// (1 / 2: padding 0, S >= 3).  *M = output pixels, *nx = input elements, *So = the output side
static int check_shape(bool valid, int B, int S, int CI, int CO, int step, long long* M, long long* nx, int* So) {
  if (B <= 0 || S < (valid ? 3 : 1) || CI <= 0 || CO <= 0 || CI % 32 || CO % 32) return HDN_E_SHAPE;
  if (step != 1 && step != 2 && (valid || step != 4)) return HDN_E_SHAPE;
  *So = valid ? (S - 3) / step + 1 : S;
  *M = (long long)B * *So * *So;
  *nx = (long long)B * S * S * CI;
  if (*nx > INT_MAX || *M * CO > INT_MAX || 9LL * CI * CO > INT_MAX) return HDN_E_LIMIT;
  return HDN_OK;
}

static int form(bool valid, int B, int S, int CI, int CO, int step) {
  long long M, nx;
  int So;
  if (const int rc = check_shape(valid, B, S, CI, CO, step, &M, &nx, &So)) return rc;
  return (int)dispatch(M, CI, CO, [&](auto cfg, int sps) -> long long {
    using C = decltype(cfg);
    return C::MT | C::NT << 4 | C::WM << 8 | C::WN << 12 | cdiv(9 * (CI / 32), sps) << 16;
  });
}

static long long workspace(bool valid, int B, int S, int CI, int CO, int step) {
  long long M, nx;
  int So;
  if (const int rc = check_shape(valid, B, S, CI, CO, step, &M, &nx, &So)) return rc;
  return dispatch(M, CI, CO, [&](auto, int sps) -> long long {
    const int Z = cdiv(9 * (CI / 32), sps);
    return Z > 1 ? Z * M * CO * 4 : 0;
  });
}

template <bool VALID>
static int run(const float* x, const void* wpacked, const float* bias, float* out, void* ws, long long ws_bytes, int B, int S, int CI, int CO, int step,
               int relu, int act_domain, void* stream) {
  if (!x || !wpacked || !out) return HDN_E_NULL;
  if ((relu != 0 && relu != 1) || (act_domain != 0 && act_domain != 1)) return HDN_E_SHAPE;
  long long M, nx;
  int So;
  if (const int rc = check_shape(VALID, B, S, CI, CO, step, &M, &nx, &So)) return rc;
  const long long nout = M * CO;
  if (bytes_overlap(out, nout * 4, x, nx * 4)) return HDN_E_ALIAS;
  if (!aligned16(x) || !aligned16(wpacked) || !aligned16(out) || (bias && !aligned16(bias))) return HDN_E_LIMIT;
  if (const int rc = check_workspace(ws, ws_bytes, workspace(VALID, B, S, CI, CO, step), x, nx * 4, out, nout * 4)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (const int rr = check_fp16_range(x, nx, s, act_domain)) return rr;
  return (int)dispatch(M, CI, CO, [&](auto cfg, int sps) -> long long {
    using C = decltype(cfg);
    return by_domain(act_domain, [&](auto sd) {
      return launch<C, decltype(sd)::value, VALID>(x, wpacked, bias, out, static_cast<float*>(ws), (int)M, S, So, step, CI, CO, relu, sps, s);
    });
  });
}

// ---- dgrad of the valid stride-1 convolution (hdn_conv3x3v_dgrad_f32): M = B S^2 pixels of gx, K = 9 CO, N = CI
static int dgrad_shape(int B, int S, int CI, int CO, long long* M, long long* ndy) {
  if (B <= 0 || S < 3 || CI <= 0 || CO <= 0 || CI % 32 || CO % 32) return HDN_E_SHAPE;
  *M = (long long)B * S * S;
  *ndy = (long long)B * (S - 2) * (S - 2) * CO;
  if (*M * CI > INT_MAX || *ndy > INT_MAX || 9LL * CI * CO > INT_MAX) return HDN_E_LIMIT;
  return HDN_OK;
}

static int dgrad_form(int B, int S, int CI, int CO) {
  long long M, ndy;
  if (const int rc = dgrad_shape(B, S, CI, CO, &M, &ndy)) return rc;
  return (int)dispatch(M, CO, CI, [&](auto cfg, int sps) -> long long {
    using C = decltype(cfg);
    return C::MT | C::NT << 4 | C::WM << 8 | C::WN << 12 | cdiv(9 * (CO / 32), sps) << 16;
  });
}

static long long dgrad_workspace(int B, int S, int CI, int CO) {
  long long M, ndy;
  if (const int rc = dgrad_shape(B, S, CI, CO, &M, &ndy)) return rc;
  return dispatch(M, CO, CI, [&](auto, int sps) -> long long {
    const int Z = cdiv(9 * (CO / 32), sps);
    return Z > 1 ? Z * M * CI * 4 : 0;
  });
}

static int dgrad_run(const float* dy, const void* wpacked_t, const int* expp, float* gx, void* ws, long long ws_bytes, int B, int S, int CI, int CO,
                     void* stream) {
  if (!dy || !wpacked_t || !expp || !gx) return HDN_E_NULL;
  long long M, ndy;
  if (const int rc = dgrad_shape(B, S, CI, CO, &M, &ndy)) return rc;
  const long long ngx = M * CI;
  if (bytes_overlap(gx, ngx * 4, dy, ndy * 4) || bytes_overlap(gx, ngx * 4, expp, 4)) return HDN_E_ALIAS;
  if (!aligned16(dy) || !aligned16(wpacked_t) || !aligned16(gx)) return HDN_E_LIMIT;
  if (const int rc = check_workspace(ws, ws_bytes, dgrad_workspace(B, S, CI, CO), dy, ndy * 4, gx, ngx * 4)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return (int)dispatch(M, CO, CI, [&](auto cfg, int sps) -> long long {
    using C = decltype(cfg);
    const int steps = 9 * (CO / 32), Z = cdiv(steps, sps), tm = cdiv((int)M, C::BM);
    const dim3 grid((unsigned)((long long)tm * (CI / C::BN)), (unsigned)Z);
    const u32x4* w = static_cast<const u32x4*>(wpacked_t);
    if (Z == 1) {
      hipLaunchKernelGGL((conv3x3_dgrad_kernel<C, true>), grid, dim3(256), 0, s, dy, w, expp, gx, (int)M, S - 2, S, CO, CI, tm, sps);
      return launch_status();
    }
    hipLaunchKernelGGL((conv3x3_dgrad_kernel<C, false>), grid, dim3(256), 0, s, dy, w, expp, static_cast<float*>(ws), (int)M, S - 2, S, CO, CI, tm, sps);
    if (const int rc = launch_status()) return rc;
    return finish_slices(static_cast<float*>(ws), Z, nullptr, 0, gx, ngx, CI, s);
  });
}

}  // namespace c3d
}  // namespace hdn

// the launch form dispatch() picks for a problem, for tests and profiles: MT | NT << 4 | WM << 8 | WN << 12 | (K slices Z) << 16.  Host only.
extern "C" int hdn_conv3x3d_form(int B, int S, int CI, int CO, int dilation) { return hdn::c3d::form(false, B, S, CI, CO, dilation); }

extern "C" long long hdn_conv3x3d_workspace_bytes(int B, int S, int CI, int CO, int dilation) { return hdn::c3d::workspace(false, B, S, CI, CO, dilation); }

// wpacked (hdn_pack_conv3x3d_f32): [CO / 32 n tiles][9 taps][CI / 32 chunks][2 k steps t][2 pieces][k half g][32 n][8] fp16; element e of lane (g, n) =
// piece of w[co = 32 tile + n][ci = 32 chunk + 16 g + 8 t + e][tap = 3 ky + kx]
extern "C" int hdn_conv3x3d_f32(const float* x, const void* wpacked, const float* bias, float* out, void* ws, long long ws_bytes, int B, int S, int CI,
                                int CO, int dilation, int relu, int act_domain, void* stream) {
  return hdn::c3d::run<false>(x, wpacked, bias, out, ws, ws_bytes, B, S, CI, CO, dilation, relu, act_domain, stream);
}

// ------------------------------------------------------------------------------- padding 0, stride 1 / 2 (hdn_conv3x3v_f32), on the same stream
extern "C" int hdn_conv3x3v_form(int B, int S, int CI, int CO, int stride) { return hdn::c3d::form(true, B, S, CI, CO, stride); }

extern "C" long long hdn_conv3x3v_workspace_bytes(int B, int S, int CI, int CO, int stride) { return hdn::c3d::workspace(true, B, S, CI, CO, stride); }

extern "C" int hdn_conv3x3v_f32(const float* x, const void* wpacked, const float* bias, float* out, void* ws, long long ws_bytes, int B, int S, int CI,
                                int CO, int stride, int relu, int act_domain, void* stream) {
  return hdn::c3d::run<true>(x, wpacked, bias, out, ws, ws_bytes, B, S, CI, CO, stride, relu, act_domain, stream);
}

// ------------------------------------------------------------------------------- the input gradient of hdn_conv3x3v_f32 at stride 1: the FULL pixel map
extern "C" int hdn_conv3x3v_dgrad_form(int B, int S, int CI, int CO) { return hdn::c3d::dgrad_form(B, S, CI, CO); }

extern "C" long long hdn_conv3x3v_dgrad_workspace_bytes(int B, int S, int CI, int CO) { return hdn::c3d::dgrad_workspace(B, S, CI, CO); }

extern "C" int hdn_conv3x3v_dgrad_f32(const float* dy, const void* wpacked_t, const int* exp, float* gx, void* ws, long long ws_bytes, int B, int S, int CI,
                                      int CO, void* stream) {
  return hdn::c3d::dgrad_run(dy, wpacked_t, exp, gx, ws, ws_bytes, B, S, CI, CO, stream);
}
