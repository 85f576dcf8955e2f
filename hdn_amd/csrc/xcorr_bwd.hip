// Backward of the depthwise cross-correlations (plain and log-polar circular) for gfx950: hdn_xcorr_depthwise_bwd_f32.
//
// Per plane p = b*C + c, with ph = Hx/2, pw = Wx/2 for the circular variant (0 for the plain one), HP = Hx + 2 ph, WP = Wx + 2 pw,
// Ho = HP - Hk + 1, Wo = WP - Wk + 1 and the padded plane xp[P][Q] = x[(P - ph) mod Hx][clamp(Q - pw, 0, Wx - 1)]:
//   forward   out[i][j] = sum_{u,v} xp[i+u][j+v] k[u][v]                            (csrc/xcorr.hip; hdn/core/xcorr.py:37-61)
//   gk[u][v]  = sum_{i,j} g[i][j] xp[i+u][j+v]                                      the same valid correlation with g as the taps
//   gxp[P][Q] = sum_{u,v} g[P-u][Q-v] k[u][v]  over 0 <= P-u < Ho, 0 <= Q-v < Wo    the gradient on the padded plane
//   gx[r][s]  = sum of gxp[P][Q] over the padded positions that are copies of (r, s):
//               P in {r + ph - Hx, r + ph, r + ph + Hx} within [0, HP);  Q = s + pw, widened to [0, pw] at s == 0 and to [pw + Wx - 1, WP) at
//               s == Wx - 1 (plain variant: the one position (r, s), gx = gxp).
//
// Gather form, no atomics: every gx element and every gk tap has ONE owner that adds its terms in a fixed order, so two calls are bit-equal and a
// plane's result does not depend on how many planes the launch has.  fp32 __builtin_fmaf chains throughout; the pad is never written to HBM.
//   gx  one thread per source element (r, s): gxp of its preimages added in ascending (P, Q), each gxp one chain over its taps in ascending (u, v).
//   gk  one wave per tap (eight taps in one pass over the outputs): lane l adds the outputs l, l + 64, ... in one chain per tap, and the 64 partial
//       sums of a tap meet in a fixed shuffle tree (32, 16, 8, 4, 2, 1; reduce_taps runs the eight trees of a pass together).  (At 5x5 (x) 29x29 a tap
//       has 625 terms: a thread per tap would leave 231 of 256 lanes idle.)
// One workgroup per plane, two forms chosen on the host (hdn_xcorr_bwd_form):
//   0  LDS form: g, k and (when gk is asked for) the padded plane are staged in LDS through the index map; (HP WP + Hk Wk + Ho Wo) 4 bytes <= 60 KiB
//      (static-size dynamic LDS below 64 KiB: no attribute opt-in).  The two training shapes take 6.0 KB (5x5 (x) 29x29) and 3.9 KB (13x13 circular).
//      gk comes first; the circular variant then puts gxp where xp was.
//   1  global form: the same loops read x, k and g from global memory (L2) through the same index functions.  There is no place for gxp, so the
//      circular gx computes each gxp where it is gathered: an element of column 0 or Wx - 1 costs up to 2 (pw + 1) min(Hk, Ho) min(Wk, Wo)
//      multiply-adds in one thread (docs/KERNELS.md "xcorr_bwd" states what that means at large planes).
// Both forms add the same terms in the same order: their results are bit-equal.
#include "hdn_common.h"

namespace hdn {
namespace xbwd {

constexpr int LDS_LIMIT_BYTES = 60 * 1024;
constexpr int TAPS = 8;  // taps of gk a wave accumulates in one pass over the outputs

// source row of padded row r (rows wrap once: HP < 2 HX), as in xcorr_generic_kernel
__device__ __forceinline__ int circ_row(int r, int HX) {
  int sr = r - HX / 2;
  return sr < 0 ? sr + HX : (sr >= HX ? sr - HX : sr);
}
// float offset inside the plane x of the padded position (P, Q)
__device__ __forceinline__ int pad_index(int P, int Q, int HX, int WX, int circ) {
  const int sr = circ ? circ_row(P, HX) : P;
  const int sc = circ ? min(max(Q - WX / 2, 0), WX - 1) : Q;
  return sr * WX + sc;
}

// The shuffle tree of gk for the TAPS = 8 partial sums of a lane at once.  Per tap it is the tree 32, 16, 8, 4, 2, 1 (lane l takes lane l + offset), whose
// root is lane 0; here the eight trees share their first three levels: at offset 32 a lane of the lower half keeps taps 0..3 and hands taps 4..7 to its
// partner (which keeps those), at 16 and 8 likewise, so that lane l then holds the level-3 sum of position l & 7 of tap l >> 3, and the last three
// levels run once for all taps.  The same pairs are added at every level (a + b == b + a), so every tap gets the bits of its own tree, with 10
// cross-lane moves instead of 48.  Returns tap (lane >> 3)'s sum in the lanes with (lane & 7) == 0.
__device__ __forceinline__ float reduce_taps(const float (&acc)[TAPS], int lane) {
  static_assert(TAPS == 8 && HDN_WAVE == 64, "three halving levels, then eight lanes per tap");
  float b[4], c[2];
  const bool h32 = lane & 32, h16 = lane & 16, h8 = lane & 8;
#pragma unroll
  for (int m = 0; m < 4; ++m) b[m] = (h32 ? acc[m + 4] : acc[m]) + __shfl_xor(h32 ? acc[m] : acc[m + 4], 32, HDN_WAVE);
#pragma unroll
  for (int m = 0; m < 2; ++m) c[m] = (h16 ? b[m + 2] : b[m]) + __shfl_xor(h16 ? b[m] : b[m + 2], 16, HDN_WAVE);
  float d = (h8 ? c[1] : c[0]) + __shfl_xor(h8 ? c[0] : c[1], 8, HDN_WAVE);
  d += __shfl_down(d, 4, HDN_WAVE);
  d += __shfl_down(d, 2, HDN_WAVE);
  d += __shfl_down(d, 1, HDN_WAVE);
  return d;
}

struct Geometry {
  int ph, pw, HP, WP, HO, WO;
};
__host__ __device__ inline Geometry geometry(int circular, int Hx, int Wx, int Hk, int Wk) {
  Geometry G;
  G.ph = circular ? Hx / 2 : 0;
  G.pw = circular ? Wx / 2 : 0;
  G.HP = Hx + 2 * G.ph;
  G.WP = Wx + 2 * G.pw;
  G.HO = G.HP - Hk + 1;
  G.WO = G.WP - Wk + 1;
  return G;
}

// the forward's xcorr_check (csrc/xcorr.hip), restated
static int check(int B, int C, int Hx, int Wx, int Hk, int Wk, int circular) {
  if (B <= 0 || C <= 0 || Hx <= 0 || Wx <= 0 || Hk <= 0 || Wk <= 0) return HDN_E_SHAPE;
  const int HP = circular ? Hx + 2 * (Hx / 2) : Hx, WP = circular ? Wx + 2 * (Wx / 2) : Wx;
  if (Hk > HP || Wk > WP) return HDN_E_SHAPE;
  if (Hx > 4096 || Wx > 4096) return HDN_E_LIMIT;
  return HDN_OK;
}

static size_t lds_bytes(const Geometry& G, int Hk, int Wk) {
  return (size_t(G.HP) * G.WP + size_t(Hk) * Wk + size_t(G.HO) * G.WO) * sizeof(float);
}

template <bool USE_LDS>
__global__ __launch_bounds__(HDN_BLOCK) void xcorr_bwd_kernel(const float* __restrict__ x, const float* __restrict__ k,
                                                               const float* __restrict__ gout, float* __restrict__ gx,
                                                               float* __restrict__ gk, int HX, int WX, int HK, int WK, int circ) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x;
  const size_t plane = blockIdx.x;
  const Geometry G = geometry(circ, HX, WX, HK, WK);
  const int HP = G.HP, WP = G.WP, HO = G.HO, WO = G.WO;
  const int NX = HX * WX, NK = HK * WK, NO = HO * WO;
  const float* __restrict__ xg = x + plane * NX;
  const float* __restrict__ kg = k + plane * NK;
  const float* __restrict__ gg = gout + plane * NO;

  // LDS image: g [HO][WO], k [HK][WK], xp [HP][WP] (the padded plane, only when gk is asked for)
  const float* gs = gg;
  const float* ks = kg;
  if constexpr (USE_LDS) {
    float* sg = smem;
    float* sk = smem + NO;
    float* sxp = sk + NK;
    for (int idx = tid; idx < NO; idx += HDN_BLOCK) sg[idx] = gg[idx];
    for (int idx = tid; idx < NK; idx += HDN_BLOCK) sk[idx] = kg[idx];
    if (gk) {
      for (int idx = tid; idx < HP * WP; idx += HDN_BLOCK) {
        const int r = idx / WP, c = idx - r * WP;
        sxp[idx] = xg[pad_index(r, c, HX, WX, circ)];
      }
    }
    __syncthreads();
    gs = sg;
    ks = sk;
  }

  // ---- gk: a wave per group of TAPS taps, lanes stride over the outputs, fixed shuffle tree per tap ----------
  // A lane reads g[o] and its index once for the TAPS taps of the group (their offsets into xp are wave-uniform); every tap still has its own chain
  // per lane and its own tree, so the grouping changes no bit.  The taps a last group lacks repeat the last tap and are not stored.
  if (gk) {
    float* __restrict__ gkp = gk + plane * NK;
    const int lane = tid & (HDN_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int di = HDN_WAVE / WO, dj = HDN_WAVE - di * WO;  // output o + 64 is (i + di, j + dj), with a carry
    const int i0 = lane / WO, j0 = lane - i0 * WO;
    for (int t0 = wave * TAPS; t0 < NK; t0 += (HDN_BLOCK / HDN_WAVE) * TAPS) {  // wave-uniform
      int tu[TAPS], tv[TAPS];
#pragma unroll
      for (int q = 0; q < TAPS; ++q) {
        const int t = min(t0 + q, NK - 1);
        tu[q] = t / WK;
        tv[q] = t - tu[q] * WK;
      }
      float acc[TAPS];
#pragma unroll
      for (int q = 0; q < TAPS; ++q) acc[q] = 0.f;
      int i = i0, j = j0;
      for (int o = lane; o < NO; o += HDN_WAVE) {
        const float gv = gs[o];
        if constexpr (USE_LDS) {
          const float* xb = smem + NO + NK + i * WP + j;
#pragma unroll
          for (int q = 0; q < TAPS; ++q) acc[q] = __builtin_fmaf(gv, xb[tu[q] * WP + tv[q]], acc[q]);
        } else {
#pragma unroll
          for (int q = 0; q < TAPS; ++q) acc[q] = __builtin_fmaf(gv, xg[pad_index(i + tu[q], j + tv[q], HX, WX, circ)], acc[q]);
        }
        j += dj;
        i += di;
        if (j >= WO) {
          j -= WO;
          ++i;
        }
      }
      const float a = reduce_taps(acc, lane);
      const int q = lane >> 3;
      if ((lane & 7) == 0 && t0 + q < NK) gkp[t0 + q] = a;
    }
  }

  // ---- gx: one thread per source element, its preimages in ascending (P, Q) ---------------------------------
  // gx[r][s] = 0 + gxp(P1, Q1) + gxp(P2, Q2) + ... (plain adds), gxp(P, Q) one fma chain from 0 over its taps in ascending (u, v).  The plain variant has
  // one preimage, and 0 + gxp == gxp bit for bit (a chain that starts at +0 never ends at -0).  The circular LDS form computes every gxp once, one thread
  // per PADDED position into the (now dead) image of xp - an edge column has pw + 1 preimages per row, which would otherwise make every wave wait for its
  // edge lanes - and then gathers; the global form computes each gxp where it is gathered.  Same terms, same order, same bits in both.
  if (gx) {
    float* __restrict__ gxo = gx + plane * NX;
    const auto gxp = [&](int P, int Q) {
      const int u0 = max(0, P - HO + 1), u1 = min(HK - 1, P);
      const int v0 = max(0, Q - WO + 1), v1 = min(WK - 1, Q);
      float part = 0.f;
      for (int u = u0; u <= u1; ++u) {
        const float* gr = gs + (P - u) * WO + Q;
        const float* kr = ks + u * WK;
        for (int v = v0; v <= v1; ++v) part = __builtin_fmaf(gr[-v], kr[v], part);
      }
      return part;
    };
    if (!circ) {
      for (int e = tid; e < NX; e += HDN_BLOCK) {
        const int r = e / WX;
        gxo[e] = gxp(r, e - r * WX);
      }
    } else {
      float* sp = smem + NO + NK;  // LDS form: gxp [HP][WP] over the image of xp
      if constexpr (USE_LDS) {
        __syncthreads();  // every wave is done reading xp
        for (int idx = tid; idx < HP * WP; idx += HDN_BLOCK) {
          const int P = idx / WP;
          sp[idx] = gxp(P, idx - P * WP);
        }
        __syncthreads();
      }
      for (int e = tid; e < NX; e += HDN_BLOCK) {
        const int r = e / WX, s = e - r * WX;
        const int qlo = s == 0 ? 0 : s + G.pw;
        const int qhi = s == WX - 1 ? WP - 1 : s + G.pw;
        float acc = 0.f;
        for (int t = -1; t <= 1; ++t) {
          const int P = r + G.ph + t * HX;
          if (P < 0 || P >= HP) continue;
          for (int Q = qlo; Q <= qhi; ++Q) {
            if constexpr (USE_LDS) acc += sp[P * WP + Q];
            else acc += gxp(P, Q);
          }
        }
        gxo[e] = acc;
      }
    }
  }
}

}  // namespace xbwd
}  // namespace hdn

extern "C" {

int hdn_xcorr_bwd_form(int circular, int Hx, int Wx, int Hk, int Wk) {
  const int rc = hdn::xbwd::check(1, 1, Hx, Wx, Hk, Wk, circular);
  if (rc) return rc;
  const hdn::xbwd::Geometry G = hdn::xbwd::geometry(circular, Hx, Wx, Hk, Wk);
  return hdn::xbwd::lds_bytes(G, Hk, Wk) <= size_t(hdn::xbwd::LDS_LIMIT_BYTES) ? 0 : 1;
}

int hdn_xcorr_depthwise_bwd_f32(const float* x, const float* k, const float* gout, float* gx, float* gk, int circular,
                                int B, int C, int Hx, int Wx, int Hk, int Wk, void* stream) {
  using namespace hdn;
  if (!x || !k || !gout || (!gx && !gk)) return HDN_E_NULL;
  const int rc = xbwd::check(B, C, Hx, Wx, Hk, Wk, circular);
  if (rc) return rc;
  if (gx && (gx == x || gx == k || gx == gout)) return HDN_E_ALIAS;
  if (gk && (gk == x || gk == k || gk == gout || gk == gx)) return HDN_E_ALIAS;
  // the forward's plane-count limits (xcorr_dispatch_)
  const long long planes_ll = (long long)B * C;
  if (planes_ll > 0x7fffffffLL / 4) return HDN_E_LIMIT;
  const int planes = (int)planes_ll;
  const xbwd::Geometry G = xbwd::geometry(circular, Hx, Wx, Hk, Wk);
  if ((long long)planes * G.HP * G.WP > 0x7fffffffLL) return HDN_E_LIMIT;
  const size_t lds = xbwd::lds_bytes(G, Hk, Wk);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (lds <= size_t(xbwd::LDS_LIMIT_BYTES)) {
    hipLaunchKernelGGL(xbwd::xcorr_bwd_kernel<true>, dim3(planes), dim3(HDN_BLOCK), lds, st, x, k, gout, gx, gk, Hx, Wx, Hk, Wk,
                       circular ? 1 : 0);
  } else {
    hipLaunchKernelGGL(xbwd::xcorr_bwd_kernel<false>, dim3(planes), dim3(HDN_BLOCK), 0, st, x, k, gout, gx, gk, Hx, Wx, Hk, Wk,
                       circular ? 1 : 0);
  }
  return launch_status();
}

}  // extern "C"
