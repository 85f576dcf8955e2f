// conv3x3_train.hip — what training the heads' Conv2d(CI, CO, 3, bias=False) (hdn/models/head/ban.py:55-64, ban_lp.py:17-26: stride 1, padding 0)
// needs beside the forward (hdn_conv3x3v_f32, conv3x3d.hip) and the input gradient (hdn_conv3x3v_dgrad_f32, the same kernel's FULL pixel map):
//
//   hdn_pack_conv3x3d_dev_f32   the weight stream of conv3x3d.hip built ON THE DEVICE from plain [CO][CI][3][3] fp32: a trained weight changes every
//                               step (in place, by a replayed optimizer step), so its stream is rebuilt per call, inside the captured graph.
//                               mode 0: byte for byte hdn_pack_conv3x3d_f32's stream; mode 1: the stream of w'[ci][co][ky][kx] = w[co][ci][2-ky][2-kx],
//                               the dgrad operand.
//   hdn_grad_scale_f32          the exponent e with amax|g| 2^e in [2^14, 2^15): gradients are split as g 2^e, not with the activations' fixed 2^-8
//                               (a mean loss's gradient is 1e-6 and smaller: its first fp16 piece would be subnormal or zero).
//   hdn_conv3x3v_wgrad_f32      gw[co][ci][ky][kx] = sum_{b,oy,ox} dy[b,oy,ox,co] x[b,oy+ky,ox+kx,ci] on the matrix cores.
//
// wgrad is a GEMM with M = CO (A = dy), N = CI (B = x), K = the pixel axis, per tap.  K is the STRIDED axis of both channels-last operands, and an MFMA
// fragment is 8 consecutive k of one row / column: the stager transposes in REGISTERS.  A staging item is one pixel position x 4 channels of EIGHT IMAGES
// (8 16-byte loads, each coalesced over the lanes' channel quads); the 8 images of a channel are split pairwise and stored as one 16-byte LDS slot, so
// an MFMA fragment is one conflict-free ds_read_b128 and — the k block being 8 images at ONE pixel — a tap is a whole-slot offset in the x image.
// (ds_read_b64_tr_b16 would transpose on the read side instead; the register form costs nothing here, the 8 loads of an item being in registers anyway.)
// A k step of v_mfma_f32_32x32x16_f16 is 2 pixels x 8 images.  Batches that are no multiple of 8 pad with zero pieces.
//
// Workgroup = W waves (W = 4 / 2 / 1: the largest that divides CO / 32), one 32 x 32 (co, ci) tile x all NINE taps per wave (288 accumulator registers),
// the waves side by side in co and sharing the x image.  K walks in UNITS of (8 images, one output row), a unit in segments of 8 output pixels: the
// dy segment [8 px][32 W co] and its x halo [3 rows][10 px][32 ci] are staged once and serve all nine taps.  K is split over grid.y into Z slices of
// whole units (units per slice from (B, S, CI, CO) only); every slice writes its joined partial [CO][CI][3][3] to the workspace and finish_slices
// (epilogue.hip) adds them in slice order: deterministic, no atomics.
#include <climits>

#include "hdn_common.h"
#include "mfma_split.h"
#include "reduce.h"

namespace hdn {
namespace c3t {
using namespace hdn::mc;

// ----------------------------------------------------------------------------------------------------------------------------------- device packer
// one thread per (n tile, tap, chunk, k step t, k half g, n, e) of the stream = per weight; both pieces
__global__ __launch_bounds__(HDN_BLOCK) void pack_kernel(const float* __restrict__ w, _Float16* __restrict__ out, int* __restrict__ bad, int COp, int CIp,
                                                         int mode, int total) {
  const int idx = blockIdx.x * HDN_BLOCK + threadIdx.x;
  if (idx >= total) return;
  const int chunks = CIp >> 5;
  const int e = idx & 7, n = (idx >> 3) & 31, g = (idx >> 8) & 1, t = (idx >> 9) & 1;
  int r = idx >> 10;
  const int chunk = r % chunks;
  r /= chunks;
  const int tap = r % 9, nt = r / 9;
  const int cop = 32 * nt + n, cip = 32 * chunk + 16 * g + 8 * t + e;                // indices of the packed (possibly transposed) weight
  const float v = mode ? w[((size_t)cip * COp + cop) * 9 + (8 - tap)] : w[((size_t)cop * CIp + cip) * 9 + tap];
  if (bad && !(fabsf(v) < 65504.0f)) atomicAdd(bad, 1);                             // the host packer's range rule, counted instead of raised
  const _Float16 h = static_cast<_Float16>(v);
  const float res = (v - static_cast<float>(h)) * LO_SCALE;
  const _Float16 l = static_cast<_Float16>(res);
  const size_t o = ((((size_t)nt * 9 + tap) * chunks + chunk) * 2 + t) * 2, in = (size_t)(g * 32 + n) * 8 + e;
  out[(o + 0) * 512 + in] = h;
  out[(o + 1) * 512 + in] = l;
}

// ------------------------------------------------------------------------------------------------------------------------------------ grad scale
// max over |g| AS BIT PATTERNS (an integer max: any order gives the same answer; inf / NaN patterns are the largest), then the exponent rule
__global__ __launch_bounds__(HDN_BLOCK) void amax_bits_kernel(const float* __restrict__ gp, long long n, unsigned* __restrict__ acc) {
  const long long n4 = n >> 2, stride = (long long)gridDim.x * HDN_BLOCK;
  unsigned m = 0;
  const u32x4* g4 = reinterpret_cast<const u32x4*>(gp);
  for (long long i = (long long)blockIdx.x * HDN_BLOCK + threadIdx.x; i < n4; i += stride) {
    const u32x4 v = g4[i];
    m = max(max(m, v.x & 0x7fffffffu), max(v.y & 0x7fffffffu, max(v.z & 0x7fffffffu, v.w & 0x7fffffffu)));
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) m = max(m, __float_as_uint(gp[(n4 << 2) + threadIdx.x]) & 0x7fffffffu);
  m = wave_max(m);
  __shared__ unsigned part[BLOCK_WAVES];
  if (lane_id() == 0) part[wave_id()] = m;
  __syncthreads();
  if (threadIdx.x == 0) {                                  // one atomic per workgroup: thousands on one address cost more than the pass itself
    m = max(max(part[0], part[1]), max(part[2], part[3]));
    if (m) atomicMax(acc, m);
  }
}

// e = 141 - (exponent field of amax): amax 2^e in [2^14, 2^15).  0 for amax = 0, inf, NaN; a subnormal amax counts as the smallest normal.
__host__ __device__ inline int exponent_rule(unsigned bits) {
  const int f = (int)(bits >> 23);
  if (bits == 0 || f == 255) return 0;
  return 141 - (f < 1 ? 1 : f);
}

__global__ void exponent_kernel(int* acc) { *acc = exponent_rule((unsigned)*acc); }

// ----------------------------------------------------------------------------------------------------------------------------------------- wgrad
constexpr int PX = 8;            // output pixels per staged segment
constexpr int XC = PX + 2;       // x columns of its halo
constexpr int FILL = 256, MAX_Z = 16;

// LDS slot of channel c of a tile of NCH channels, staged four at a time: the four channels of a lane's 16-byte load go to slots NCH / 4 apart, so
// that for each of them consecutive lanes write consecutive slots (a ds_write_b128 of 8 lanes = one 128-byte bank row).  The inverse is channel_of.
__device__ __forceinline__ int slot_of(int c, int nch) { return (c & 3) * (nch >> 2) + (c >> 2); }
__device__ __forceinline__ int channel_of(int s, int nch) { return 4 * (s % (nch >> 2)) + s / (nch >> 2); }

// 8 images x 4 channels (v[j] = image j) -> the four channels' 16-byte slots of the two piece planes; GE: scale 2^ge first (gradient), else 2^-8
template <bool GRADIENT>
__device__ __forceinline__ void split_store8(const f4 (&v)[8], int ge, u32x4* p0dst, u32x4* p1dst, int slot_stride) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    unsigned q0[4], q1[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f2 pr{v[2 * j][c], v[2 * j + 1][c]};
      if constexpr (GRADIENT) {
        pr = f2{ldexpf(pr.x, ge), ldexpf(pr.y, ge)};
        split2<true>(pr, q0[j], q1[j]);
      } else {
        split2<false>(pr, q0[j], q1[j]);
      }
    }
    p0dst[c * slot_stride] = u32x4{q0[0], q0[1], q0[2], q0[3]};
    p1dst[c * slot_stride] = u32x4{q1[0], q1[1], q1[2], q1[3]};
  }
}

template <int W, bool FINAL>
__global__ __launch_bounds__(64 * W) void wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy, const int* __restrict__ expp,
                                                        float* __restrict__ dst, int B, int S, int CI, int CO, int units, int ups) {
  constexpr int NCO = 32 * W, THREADS = 64 * W;
  __shared__ u32x4 dyL[2][PX][NCO];        // [piece][pixel][co slot]: 8 images of one (pixel, channel) per slot
  __shared__ u32x4 xL[2][3][XC][32];       // [piece][row][column][ci slot]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, g = lane >> 5;
  const int So = S - 2, nco = CO / NCO;
  const int co0 = ((int)blockIdx.x % nco) * NCO, ci0 = ((int)blockIdx.x / nco) * 32;
  const int ge = *expp;
  const int u0 = FINAL ? 0 : (int)blockIdx.y * ups, u1 = FINAL ? units : min(units, u0 + ups);

  f32x16 hi[9], lo[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) hi[t][r] = lo[t][r] = 0.f;

  for (int u = u0; u < u1; ++u) {
    const int bg = u / So, oy = u - bg * So, b0 = 8 * bg;
    for (int ox0 = 0; ox0 < So; ox0 += PX) {
      __syncthreads();                                                       // the previous segment's reads are done
      {  // dy segment: THREADS items = 8 pixels x NCO / 4 channel quads
        const int px = tid / (NCO / 4), cq = tid % (NCO / 4);
        const bool pok = ox0 + px < So;
        f4 v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const bool ok = pok && b0 + j < B;
          const size_t off = ((((size_t)(ok ? b0 + j : 0) * So + oy) * So + (ok ? ox0 + px : 0)) * CO) + co0 + 4 * cq;
          v[j] = ok ? *reinterpret_cast<const f4*>(dy + off) : f4{0.f, 0.f, 0.f, 0.f};
        }
        split_store8<true>(v, ge, &dyL[0][px][cq], &dyL[1][px][cq], NCO / 4);
      }
      for (int it = tid; it < 3 * XC * 8; it += THREADS) {                   // x halo: 3 rows x 10 columns x 8 channel quads
        const int cq = it & 7, rc = it >> 3, row = rc / XC, col = rc - row * XC;
        const bool cok = ox0 + col < S;
        f4 v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const bool ok = cok && b0 + j < B;
          const size_t off = ((((size_t)(ok ? b0 + j : 0) * S + oy + row) * S + (ok ? ox0 + col : 0)) * CI) + ci0 + 4 * cq;
          v[j] = ok ? *reinterpret_cast<const f4*>(x + off) : f4{0.f, 0.f, 0.f, 0.f};
        }
        split_store8<false>(v, 0, &xL[0][row][col][cq], &xL[1][row][col][cq], 8);
      }
      __syncthreads();
#pragma unroll
      for (int ks = 0; ks < PX / 2; ++ks) {                                  // k step = pixels 2 ks, 2 ks + 1 (k half g) x 8 images
        const int px = 2 * ks + g;
        const u32x4 a0 = dyL[0][px][32 * wave + li], a1 = dyL[1][px][32 * wave + li];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            const u32x4 b0v = xL[0][ky][px + kx][li], b1v = xL[1][ky][px + kx][li];
            const int t = 3 * ky + kx;
            hi[t] = mfma(a0, b0v, hi[t]);
            lo[t] = mfma(a0, b1v, lo[t]);
            lo[t] = mfma(a1, b0v, lo[t]);
          }
      }
    }
  }

  // epilogue: register r of a lane = co slot 32 wave + d_row(r, g), ci slot li, nine taps -> plain [CO][CI][3][3]
  float* o = FINAL ? dst : dst + (size_t)blockIdx.y * CO * CI * 9;
  const int ci = ci0 + channel_of(li, 32);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int co = co0 + channel_of(32 * wave + d_row(r, g), NCO);
    float* q = o + ((size_t)co * CI + ci) * 9;
#pragma unroll
    for (int t = 0; t < 9; ++t) q[t] = ldexpf(join<true>(hi[t][r], lo[t][r]), HDN_ACT_SCALE_LOG2 - ge);
  }
}

static int wgrad_shape(int B, int S, int CI, int CO, long long* nx, long long* ndy) {
  if (B <= 0 || S < 3 || CI <= 0 || CO <= 0 || CI % 32 || CO % 32) return HDN_E_SHAPE;
  *nx = (long long)B * S * S * CI;
  *ndy = (long long)B * (S - 2) * (S - 2) * CO;
  if (*nx > INT_MAX || *ndy > INT_MAX || 9LL * CI * CO > INT_MAX) return HDN_E_LIMIT;
  return HDN_OK;
}

struct Plan {
  int W, units, ups, Z;
};
static Plan plan(int B, int S, int CI, int CO) {
  Plan p;
  p.W = CO % 128 == 0 ? 4 : CO % 64 == 0 ? 2 : 1;
  p.units = cdiv(B, 8) * (S - 2);
  const long long wgs = (long long)(CO / (32 * p.W)) * (CI / 32);
  long long z = wgs >= FILL ? 1 : (FILL + wgs - 1) / wgs;
  if (z > MAX_Z) z = MAX_Z;
  if (z > p.units) z = p.units;
  p.ups = cdiv(p.units, (int)z);
  p.Z = cdiv(p.units, p.ups);
  return p;
}

template <int W>
static int launch(const Plan& p, const float* x, const float* dy, const int* expp, float* gw, float* ws, int B, int S, int CI, int CO, hipStream_t s) {
  const dim3 grid((unsigned)((CO / (32 * W)) * (CI / 32)), (unsigned)p.Z);
  if (p.Z == 1) {
    hipLaunchKernelGGL((wgrad_kernel<W, true>), grid, dim3(64 * W), 0, s, x, dy, expp, gw, B, S, CI, CO, p.units, p.ups);
    return launch_status();
  }
  hipLaunchKernelGGL((wgrad_kernel<W, false>), grid, dim3(64 * W), 0, s, x, dy, expp, ws, B, S, CI, CO, p.units, p.ups);
  if (const int rc = launch_status()) return rc;
  return finish_slices(ws, p.Z, nullptr, 0, gw, 9LL * CO * CI, 4, s);
}

}  // namespace c3t
}  // namespace hdn

using namespace hdn;

extern "C" int hdn_pack_conv3x3d_dev_f32(const float* w, int CO, int CI, int mode, void* out, long long out_bytes, int* bad_count, void* stream) {
  if (!w || !out) return HDN_E_NULL;
  if ((mode != 0 && mode != 1) || hdn_pack_conv3x3d_bytes(CO, CI) < 0 || out_bytes != hdn_pack_conv3x3d_bytes(CO, CI)) return HDN_E_SHAPE;
  if (!aligned16(out)) return HDN_E_LIMIT;
  if (bytes_overlap(out, out_bytes, w, 36LL * CO * CI)) return HDN_E_ALIAS;
  const int total = 9 * CO * CI;
  hipLaunchKernelGGL(c3t::pack_kernel, dim3(cdiv(total, HDN_BLOCK)), dim3(HDN_BLOCK), 0, static_cast<hipStream_t>(stream), w, static_cast<_Float16*>(out),
                     bad_count, mode ? CI : CO, mode ? CO : CI, mode, total);
  return launch_status();
}

extern "C" int hdn_grad_scale_f32(const float* g, long long n, int* exp_out, void* stream) {
  if (!g || !exp_out) return HDN_E_NULL;
  if (n <= 0) return HDN_E_SHAPE;
  if (!aligned16(g)) return HDN_E_LIMIT;
  if (bytes_overlap(exp_out, 4, g, n * 4)) return HDN_E_ALIAS;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (const int rc = hip_status(hipMemsetAsync(exp_out, 0, 4, s))) return rc;
  const long long want = ((n >> 2) + HDN_BLOCK - 1) / HDN_BLOCK;
  const int blocks = (int)(want < 1 ? 1 : want > 512 ? 512 : want);
  hipLaunchKernelGGL(c3t::amax_bits_kernel, dim3(blocks), dim3(HDN_BLOCK), 0, s, g, n, reinterpret_cast<unsigned*>(exp_out));
  if (const int rc = launch_status()) return rc;
  hipLaunchKernelGGL(c3t::exponent_kernel, dim3(1), dim3(1), 0, s, exp_out);
  return launch_status();
}

// W | Z << 16: waves per workgroup (32 W output channels x 32 input channels x nine taps), K slices.  Host only.
extern "C" int hdn_conv3x3v_wgrad_form(int B, int S, int CI, int CO) {
  long long nx, ndy;
  if (const int rc = c3t::wgrad_shape(B, S, CI, CO, &nx, &ndy)) return rc;
  const c3t::Plan p = c3t::plan(B, S, CI, CO);
  return p.W | p.Z << 16;
}

extern "C" long long hdn_conv3x3v_wgrad_workspace_bytes(int B, int S, int CI, int CO) {
  long long nx, ndy;
  if (const int rc = c3t::wgrad_shape(B, S, CI, CO, &nx, &ndy)) return rc;
  const c3t::Plan p = c3t::plan(B, S, CI, CO);
  return p.Z > 1 ? 36LL * p.Z * CO * CI : 0;
}

extern "C" int hdn_conv3x3v_wgrad_f32(const float* x, const float* dy, const int* exp, float* gw, void* ws, long long ws_bytes, int B, int S, int CI,
                                      int CO, void* stream) {
  if (!x || !dy || !exp || !gw) return HDN_E_NULL;
  long long nx, ndy;
  if (const int rc = c3t::wgrad_shape(B, S, CI, CO, &nx, &ndy)) return rc;
  const long long ngw = 9LL * CO * CI;
  if (bytes_overlap(gw, ngw * 4, x, nx * 4) || bytes_overlap(gw, ngw * 4, dy, ndy * 4) || bytes_overlap(gw, ngw * 4, exp, 4)) return HDN_E_ALIAS;
  if (!aligned16(x) || !aligned16(dy) || !aligned16(gw)) return HDN_E_LIMIT;
  const c3t::Plan p = c3t::plan(B, S, CI, CO);
  const long long need = p.Z > 1 ? 36LL * p.Z * CO * CI : 0;
  if (const int rc = check_workspace(ws, ws_bytes, need, x, nx * 4, gw, ngw * 4)) return rc;
  if (need > 0 && bytes_overlap(ws, need, dy, ndy * 4)) return HDN_E_ALIAS;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (const int rr = check_fp16_range(x, nx, s, 0)) return rr;
  float* wsf = static_cast<float*>(ws);
  if (p.W == 4) return c3t::launch<4>(p, x, dy, exp, gw, wsf, B, S, CI, CO, s);
  if (p.W == 2) return c3t::launch<2>(p, x, dy, exp, gw, wsf, B, S, CI, CO, s);
  return c3t::launch<1>(p, x, dy, exp, gw, wsf, B, S, CI, CO, s);
}
