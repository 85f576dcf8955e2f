// The similarity model's training geometry between the head maps and the samplers, forward and backward, for gfx950:
//
//   hdn_point_pick_f32 / _bwd_f32     mode 0: Polar_Pick.get_polar_from_two_para_loc (hdn/models/logpolar.py:304-324)
//                                     mode 1: lp_pick (hdn/utils/point.py:35-53)
//   hdn_simi_affine_f32 / _bwd_f32    kind 0: combine_affine_c0_v2, kind 1: combine_affine_lt0 (hdn/utils/transform.py:442-523)
//   hdn_simi_warps_f32 / _bwd_f32     model_builder_e2e_unconstrained_v2.py:390-415: lp_pick, the four matrices, pred_points, aug_sear_points
//
// The formulas are in include/hdn_hip.h.  The picks and the fused form run one wave per sample (grid = B): the lanes scan the S S cells in strides of
// 64 and the butterfly of argmax_order.h leaves the same winner in every lane, so the closed form after it is wave-uniform arithmetic that lane 0
// stores.  hdn_simi_affine has nothing to scan: one thread per sample.  No LDS, no atomics; the point table is computed from (stride, S).  Each
// formula is one device function (lp_decode, lp_grads, affine_operands, affine_rows, affine_grads, poly_rows) that every entry point shares.
//
// Bounds: after the argmax best lies in [0, n) for any input (argmax_order.h), so loc[c n + best] is a read inside the map.  The backward kernels
// read best_idx from memory and compare it against [0, n) before it is used; they write grad_loc by position, never through best_idx.
#include <math.h>

#include "argmax_order.h"
#include "hdn_common.h"

#pragma clang fp contract(off)

namespace hdn {
namespace simi_geo {

// generate_points(stride, S)[i]: integers, exact in fp32 under the entry points' limits (|coordinate| <= 2^21)
__device__ __forceinline__ void point_of(int i, int S, int stride, float& px, float& py) {
  const int ori = -(S / 2) * stride;
  px = (float)(ori + stride * (i % S));
  py = (float)(ori + stride * (i / S));
}

// the winner of one sample's map, the same in every lane.  MODE 0: the raw logit of class 1; MODE 1: its fp32 softmax
template <int MODE>
__device__ __forceinline__ int pick_best(const float* __restrict__ cls, int n, int lane) {
  const auto score = [&](int i) { return MODE == 0 ? (double)cls[n + i] : (double)softmax2_class1(cls[i], cls[n + i]); };
  int best_i = argmax_start(lane, n);  // best_i in [0, n) from here on
  double best = score(best_i);
  for (int i = lane + HDN_WAVE; i < n; i += HDN_WAVE) {
    const double v = score(i);
    if (argmax_takes(v, i, best, best_i)) { best = v; best_i = i; }
  }
  wave_argmax(best, best_i);
  return best_i;
}

// lp_pick after the gather (point.py:48-52): scale = exp((px - d0 STRIDE_LP) mag), rot = (py - d2 STRIDE_LP) (2 pi / MAP_SIZE)
__device__ __forceinline__ void lp_decode(const float* __restrict__ loc_lp, int n, int best, int S, int stride, float mult, float mag,
                                          float rot_unit, float& scale, float& rot) {
  float px, py;
  point_of(best, S, stride, px, py);
  scale = expf(rn_mul(rn_sub(px, rn_mul(loc_lp[best], mult)), mag));
  rot = rn_mul(rn_sub(py, rn_mul(loc_lp[2 * n + best], mult)), rot_unit);
}

// its backward in autograd's order: exp (g result), the two scalar products, the negation of the subtraction
__device__ __forceinline__ void lp_grads(float g_scale, float g_rot, float scale, float mult, float mag, float rot_unit, float& g0, float& g2) {
  g0 = rn_mul(-rn_mul(rn_mul(g_scale, scale), mag), mult);
  g2 = rn_mul(-rn_mul(g_rot, rot_unit), mult);
}

// grad of a [B,C,S,S] map that is zero except at cell `best` of the channels c0 and c1: every element written once, by position
__device__ __forceinline__ void write_pick_grad(float* __restrict__ g, int n, int C, int best, int c0, float v0, int c1, float v1, int lane) {
  const bool ok = best >= 0 && best < n;
  for (int i = lane; i < C * n; i += HDN_WAVE) {
    float v = 0.f;
    if (ok && i == c0 * n + best) v = v0;
    if (ok && i == c1 * n + best) v = v1;
    g[i] = v;
  }
}

// the constants of the two combine_affine functions, rounded as a Python float meets an fp32 tensor
struct AffCfg {
  float k;         // out_sz / in_sz
  float half_out;  // out_sz / 2
  float half_in;   // in_sz / 2
  float in_f, out_f;
  float u_scalar, v_scalar;  // kind 0: (cx - out_sz / 2) in_sz / out_sz in double; kind 1: cx, cy
  int scale_h;
};

static AffCfg make_cfg(int kind, double cx, double cy, int scale_h, double in_sz, double out_sz) {
  AffCfg c;
  c.k = (float)(out_sz / in_sz);
  c.half_out = (float)(out_sz / 2);
  c.half_in = (float)(in_sz / 2);
  c.in_f = (float)in_sz;
  c.out_f = (float)out_sz;
  c.u_scalar = kind == 0 ? (float)((cx - out_sz / 2) * in_sz / out_sz) : (float)cx;
  c.v_scalar = kind == 0 ? (float)((cy - out_sz / 2) * in_sz / out_sz) : (float)cy;
  c.scale_h = scale_h;
  return c;
}

// what the two functions share once their operands are named: out = [[a, -c, t0], [c, a, t1]], t0 = ((-a U - (-c) V) + W0) [/ div], t1 = ((-c U - a V) + W1) [/ div]
struct AffOps {
  float sc, U, V, W0, W1;
  bool div;
};

// kind 0: cx_s = (cx - out_sz / 2) * in_sz / out_sz step by step for a tensor; kind 1: sx = nm_shift + in_sz / 2
__device__ __forceinline__ AffOps affine_operands(int kind, const AffCfg& c, float nm0, float nm1, float scale, bool vec, float cx, float cy) {
  AffOps o;
  if (kind == 0) {
    o.sc = rn_mul(c.k, scale);
    o.U = vec ? rn_div(rn_mul(rn_sub(cx, c.half_out), c.in_f), c.out_f) : c.u_scalar;
    o.V = vec ? rn_div(rn_mul(rn_sub(cy, c.half_out), c.in_f), c.out_f) : c.v_scalar;
    o.W0 = nm0;
    o.W1 = nm1;
    o.div = c.scale_h != 0;
  } else {
    o.sc = scale;
    o.U = rn_add(nm0, c.half_in);
    o.V = rn_add(nm1, c.half_in);
    o.W0 = vec ? cx : c.u_scalar;
    o.W1 = vec ? cy : c.v_scalar;
    o.div = false;
  }
  return o;
}

__device__ __forceinline__ void affine_rows(const AffOps& o, float rot, float out_f, float* m) {
  const float cc = cosf(rot), ss = sinf(rot);
  const float a = rn_mul(o.sc, cc), c = rn_mul(o.sc, ss), b = -c;
  float t0 = rn_add(rn_sub(rn_mul(-a, o.U), rn_mul(b, o.V)), o.W0);
  float t1 = rn_add(rn_sub(rn_mul(-c, o.U), rn_mul(a, o.V)), o.W1);
  if (o.div) {
    t0 = rn_div(t0, out_f);
    t1 = rn_div(t1, out_f);
  }
  m[0] = a; m[1] = b; m[2] = t0;
  m[3] = c; m[4] = a; m[5] = t1;
}

struct AffGrads {
  float sc, rot, U, V, W0, W1;
};

// d / d (sc, rot, U, V, W) of sum(G * affine_rows): t0 = -a U + c V + W0, t1 = -c U - a V + W1, a = sc cos, c = sc sin
__device__ __forceinline__ AffGrads affine_grads(const AffOps& o, float rot, float out_f, const float* G) {
  const float cc = cosf(rot), ss = sinf(rot);
  const float a = rn_mul(o.sc, cc), c = rn_mul(o.sc, ss);
  const float h0 = o.div ? rn_div(G[2], out_f) : G[2], h1 = o.div ? rn_div(G[5], out_f) : G[5];
  const float Ga = rn_sub(rn_add(G[0], G[4]), rn_add(rn_mul(o.U, h0), rn_mul(o.V, h1)));
  const float Gc = rn_add(rn_sub(G[3], G[1]), rn_sub(rn_mul(o.V, h0), rn_mul(o.U, h1)));
  AffGrads g;
  g.sc = rn_add(rn_mul(Ga, cc), rn_mul(Gc, ss));
  g.rot = rn_mul(o.sc, rn_sub(rn_mul(Gc, cc), rn_mul(Ga, ss)));
  g.U = -rn_add(rn_mul(a, h0), rn_mul(c, h1));
  g.V = rn_sub(rn_mul(c, h0), rn_mul(a, h1));
  g.W0 = h0;
  g.W1 = h1;
  return g;
}

// torch.bmm([M; 0 0 1], [x; y; 1]) of the four corners poly [4,2] -> pts [3,4]
__device__ __forceinline__ void poly_rows(const float* m, const float* __restrict__ poly, float* __restrict__ pts) {
  for (int j = 0; j < 4; ++j) {
    const float x = poly[2 * j], y = poly[2 * j + 1];
    pts[j] = rn_add(rn_add(rn_mul(m[0], x), rn_mul(m[1], y)), m[2]);
    pts[4 + j] = rn_add(rn_add(rn_mul(m[3], x), rn_mul(m[4], y)), m[5]);
    pts[8 + j] = rn_add(rn_add(rn_mul(0.f, x), rn_mul(0.f, y)), 1.f);
  }
}

template <int MODE>
__global__ __launch_bounds__(HDN_WAVE) void pick_kernel(const float* __restrict__ cls, const float* __restrict__ loc, float* __restrict__ out,
                                                        int* __restrict__ best_idx, int B, int S, int stride, float mult, float mag,
                                                        float rot_unit) {
  const int b = blockIdx.x, lane = threadIdx.x, n = S * S;
  const int best = pick_best<MODE>(cls + size_t(b) * 2 * n, n, lane);
  if (lane != 0) return;
  best_idx[b] = best;
  if (MODE == 0) {
    loc += size_t(b) * 2 * n;
    float px, py;
    point_of(best, S, stride, px, py);
    out[2 * b] = rn_sub(px, rn_mul(mult, loc[best]));
    out[2 * b + 1] = rn_sub(py, rn_mul(mult, loc[n + best]));
  } else {
    float scale, rot;
    lp_decode(loc + size_t(b) * 4 * n, n, best, S, stride, mult, mag, rot_unit, scale, rot);
    out[b] = scale;
    out[B + b] = rot;
  }
}

__global__ __launch_bounds__(HDN_WAVE) void pick_bwd_kernel(const int* __restrict__ best_idx, const float* __restrict__ grad_out,
                                                            const float* __restrict__ out, float* __restrict__ grad_loc, int B, int S, int mode,
                                                            float mult, float mag, float rot_unit) {
  const int b = blockIdx.x, lane = threadIdx.x, n = S * S;
  const int best = best_idx[b];
  if (mode == 0) {
    write_pick_grad(grad_loc + size_t(b) * 2 * n, n, 2, best, 0, rn_mul(-grad_out[2 * b], mult), 1, rn_mul(-grad_out[2 * b + 1], mult), lane);
  } else {
    float g0, g2;
    lp_grads(grad_out[b], grad_out[B + b], out[b], mult, mag, rot_unit, g0, g2);
    write_pick_grad(grad_loc + size_t(b) * 4 * n, n, 4, best, 0, g0, 2, g2, lane);
  }
}

__global__ __launch_bounds__(HDN_BLOCK) void affine_kernel(const float* __restrict__ nm, const float* __restrict__ scale, const float* __restrict__ rot,
                                                           const float* __restrict__ cx, const float* __restrict__ cy, float* __restrict__ out, int B,
                                                           int kind, AffCfg cfg) {
  const int b = blockIdx.x * HDN_BLOCK + threadIdx.x;
  if (b >= B) return;
  const bool vec = cx != nullptr;
  const AffOps o = affine_operands(kind, cfg, nm[2 * b], nm[2 * b + 1], scale[b], vec, vec ? cx[b] : 0.f, vec ? cy[b] : 0.f);
  float m[6];
  affine_rows(o, rot[b], cfg.out_f, m);
  for (int q = 0; q < 6; ++q) out[6 * size_t(b) + q] = m[q];
}

__global__ __launch_bounds__(HDN_BLOCK) void affine_bwd_kernel(const float* __restrict__ nm, const float* __restrict__ scale,
                                                               const float* __restrict__ rot, const float* __restrict__ cx,
                                                               const float* __restrict__ cy, const float* __restrict__ grad, float* __restrict__ g_nm,
                                                               float* __restrict__ g_scale, float* __restrict__ g_rot, int B, int kind, AffCfg cfg) {
  const int b = blockIdx.x * HDN_BLOCK + threadIdx.x;
  if (b >= B) return;
  const bool vec = cx != nullptr;
  const AffOps o = affine_operands(kind, cfg, nm[2 * b], nm[2 * b + 1], scale[b], vec, vec ? cx[b] : 0.f, vec ? cy[b] : 0.f);
  float G[6];
  for (int q = 0; q < 6; ++q) G[q] = grad[6 * size_t(b) + q];
  const AffGrads g = affine_grads(o, rot[b], cfg.out_f, G);
  if (g_nm) {
    g_nm[2 * b] = kind == 0 ? g.W0 : g.U;
    g_nm[2 * b + 1] = kind == 0 ? g.W1 : g.V;
  }
  if (g_scale) g_scale[b] = kind == 0 ? rn_mul(g.sc, cfg.k) : g.sc;
  if (g_rot) g_rot[b] = g.rot;
}

// cfg0 / cfg1: the constants of the kind 0 / kind 1 calls with the scalar centre (out_sz / 2, out_sz / 2) of :401-402
__global__ __launch_bounds__(HDN_WAVE) void warps_kernel(const float* __restrict__ cls_lp, const float* __restrict__ loc_lp,
                                                         const float* __restrict__ polar, const float* __restrict__ temp_cx,
                                                         const float* __restrict__ temp_cy, const float* __restrict__ search_poly,
                                                         int* __restrict__ best_idx, float* __restrict__ scale_out, float* __restrict__ rot_out,
                                                         float* __restrict__ affine_m, float* __restrict__ affine_m_lt0,
                                                         float* __restrict__ affine_m_c_aug, float* __restrict__ affine_m_lt0_aug,
                                                         float* __restrict__ pred_points, float* __restrict__ aug_sear_points, int S, int stride,
                                                         float stride_lp, float mag, float rot_unit, AffCfg cfg0, AffCfg cfg1) {
  const int b = blockIdx.x, lane = threadIdx.x, n = S * S;
  const int best = pick_best<1>(cls_lp + size_t(b) * 2 * n, n, lane);
  if (lane != 0) return;
  float scale, rot;
  lp_decode(loc_lp + size_t(b) * 4 * n, n, best, S, stride, stride_lp, mag, rot_unit, scale, rot);
  best_idx[b] = best;
  scale_out[b] = scale;
  rot_out[b] = rot;
  const float p0 = polar[2 * b], p1 = polar[2 * b + 1], tx = temp_cx[b], ty = temp_cy[b];
  float m[6];
  affine_rows(affine_operands(0, cfg0, p0, p1, scale, false, 0.f, 0.f), rot, cfg0.out_f, m);
  for (int q = 0; q < 6; ++q) affine_m[6 * size_t(b) + q] = m[q];
  affine_rows(affine_operands(0, cfg0, 0.f, 0.f, 1.f, true, tx, ty), 0.f, cfg0.out_f, m);
  for (int q = 0; q < 6; ++q) affine_m_c_aug[6 * size_t(b) + q] = m[q];
  affine_rows(affine_operands(1, cfg1, 0.f, 0.f, 1.f, true, tx, ty), 0.f, cfg1.out_f, m);
  for (int q = 0; q < 6; ++q) affine_m_lt0_aug[6 * size_t(b) + q] = m[q];
  poly_rows(m, search_poly + 8 * size_t(b), aug_sear_points + 12 * size_t(b));
  affine_rows(affine_operands(1, cfg1, p0, p1, rn_div(1.f, scale), false, 0.f, 0.f), -rot, cfg1.out_f, m);   // 1 / scale, -rot (:402)
  for (int q = 0; q < 6; ++q) affine_m_lt0[6 * size_t(b) + q] = m[q];
  poly_rows(m, search_poly + 8 * size_t(b), pred_points + 12 * size_t(b));
}

__global__ __launch_bounds__(HDN_WAVE) void warps_bwd_kernel(const int* __restrict__ best_idx, const float* __restrict__ scale_in,
                                                             const float* __restrict__ rot_in, const float* __restrict__ polar,
                                                             const float* __restrict__ search_poly, const float* __restrict__ g_scale,
                                                             const float* __restrict__ g_rot, const float* __restrict__ g_m,
                                                             const float* __restrict__ g_lt0, const float* __restrict__ g_pts,
                                                             float* __restrict__ grad_loc_lp, float* __restrict__ grad_polar, int S,
                                                             float stride_lp, float mag, float rot_unit, AffCfg cfg0, AffCfg cfg1) {
  const int b = blockIdx.x, lane = threadIdx.x, n = S * S;
  // wave-uniform arithmetic: every lane forms the same two values, then the lanes share the writing of the full-size gradient
  const float scale = scale_in[b], rot = rot_in[b], p0 = polar[2 * b], p1 = polar[2 * b + 1];
  float G0[6], G1[6];
  for (int q = 0; q < 6; ++q) {
    G0[q] = g_m ? g_m[6 * size_t(b) + q] : 0.f;
    G1[q] = g_lt0 ? g_lt0[6 * size_t(b) + q] : 0.f;
  }
  if (g_pts) {  // pred_points rows 0 and 1 = affine_m_lt0 [x; y; 1]; row 2 is constant
    const float* poly = search_poly + 8 * size_t(b);
    const float* gp = g_pts + 12 * size_t(b);
    for (int r = 0; r < 2; ++r)
      for (int j = 0; j < 4; ++j) {
        const float g = gp[4 * r + j];
        G1[3 * r] = rn_add(G1[3 * r], rn_mul(g, poly[2 * j]));
        G1[3 * r + 1] = rn_add(G1[3 * r + 1], rn_mul(g, poly[2 * j + 1]));
        G1[3 * r + 2] = rn_add(G1[3 * r + 2], g);
      }
  }
  const float inv = rn_div(1.f, scale);
  const AffGrads a0 = affine_grads(affine_operands(0, cfg0, p0, p1, scale, false, 0.f, 0.f), rot, cfg0.out_f, G0);
  const AffGrads a1 = affine_grads(affine_operands(1, cfg1, p0, p1, inv, false, 0.f, 0.f), -rot, cfg1.out_f, G1);
  // scale: its own gradient, kind 0 through sc = k scale, kind 1 through 1 / scale (-g inv inv); rot: kind 1 saw -rot
  const float gs = rn_sub(rn_add(g_scale ? g_scale[b] : 0.f, rn_mul(a0.sc, cfg0.k)), rn_mul(rn_mul(a1.sc, inv), inv));
  const float gr = rn_sub(rn_add(g_rot ? g_rot[b] : 0.f, a0.rot), a1.rot);
  if (grad_polar && lane == 0) {
    grad_polar[2 * b] = rn_add(a0.W0, a1.U);
    grad_polar[2 * b + 1] = rn_add(a0.W1, a1.V);
  }
  if (grad_loc_lp) {
    float g0, g2;
    lp_grads(gs, gr, scale, stride_lp, mag, rot_unit, g0, g2);
    write_pick_grad(grad_loc_lp + size_t(b) * 4 * n, n, 4, best_idx[b], 0, g0, 2, g2, lane);
  }
}

static int check_pick(int B, int S, int stride) {
  if (B < 1 || S < 1 || stride < 1) return HDN_E_SHAPE;
  if (S > 1024 || stride > 4096) return HDN_E_LIMIT;
  return HDN_OK;
}

static int check_affine(int B, int kind, double in_sz, double out_sz, const float* cx, const float* cy) {
  if ((cx == nullptr) != (cy == nullptr)) return HDN_E_NULL;
  if (B < 1 || (kind != 0 && kind != 1) || !(in_sz > 0) || !(out_sz > 0)) return HDN_E_SHAPE;
  return HDN_OK;
}

}  // namespace simi_geo
}  // namespace hdn

extern "C" {

int hdn_point_pick_f32(const float* cls, const float* loc, float* out, int* best_idx, int B, int S, int cls_channels, int mode, int stride, float mult,
                       double mag, double rot_unit, void* stream) {
  using namespace hdn;
  if (!cls || !loc || !out || !best_idx) return HDN_E_NULL;
  if (cls_channels != 2 || (mode != 0 && mode != 1)) return HDN_E_SHAPE;
  if (const int rc = simi_geo::check_pick(B, S, stride)) return rc;
  if (mode == 0)
    hipLaunchKernelGGL(simi_geo::pick_kernel<0>, dim3(B), dim3(HDN_WAVE), 0, static_cast<hipStream_t>(stream), cls, loc, out, best_idx, B, S, stride,
                       mult, (float)mag, (float)rot_unit);
  else
    hipLaunchKernelGGL(simi_geo::pick_kernel<1>, dim3(B), dim3(HDN_WAVE), 0, static_cast<hipStream_t>(stream), cls, loc, out, best_idx, B, S, stride,
                       mult, (float)mag, (float)rot_unit);
  return launch_status();
}

int hdn_point_pick_bwd_f32(const int* best_idx, const float* grad_out, const float* out_or_null, float* grad_loc, int B, int S, int mode, float mult,
                           double mag, double rot_unit, void* stream) {
  using namespace hdn;
  if (!best_idx || !grad_out || !grad_loc || (mode == 1 && !out_or_null)) return HDN_E_NULL;
  if (mode != 0 && mode != 1) return HDN_E_SHAPE;
  if (const int rc = simi_geo::check_pick(B, S, 1)) return rc;
  hipLaunchKernelGGL(simi_geo::pick_bwd_kernel, dim3(B), dim3(HDN_WAVE), 0, static_cast<hipStream_t>(stream), best_idx, grad_out, out_or_null,
                     grad_loc, B, S, mode, mult, (float)mag, (float)rot_unit);
  return launch_status();
}

int hdn_simi_affine_f32(const float* nm_shift, const float* scale, const float* rot, const float* cx_or_null, const float* cy_or_null, double cx_scalar,
                        double cy_scalar, float* out, int B, int kind, int scale_h, double in_sz, double out_sz, void* stream) {
  using namespace hdn;
  if (!nm_shift || !scale || !rot || !out) return HDN_E_NULL;
  if (const int rc = simi_geo::check_affine(B, kind, in_sz, out_sz, cx_or_null, cy_or_null)) return rc;
  hipLaunchKernelGGL(simi_geo::affine_kernel, dim3(cdiv(B, HDN_BLOCK)), dim3(HDN_BLOCK), 0, static_cast<hipStream_t>(stream), nm_shift, scale, rot,
                     cx_or_null, cy_or_null, out, B, kind, simi_geo::make_cfg(kind, cx_scalar, cy_scalar, scale_h, in_sz, out_sz));
  return launch_status();
}

int hdn_simi_affine_bwd_f32(const float* nm_shift, const float* scale, const float* rot, const float* cx_or_null, const float* cy_or_null,
                            double cx_scalar, double cy_scalar, const float* grad, float* grad_nm_shift_or_null, float* grad_scale_or_null,
                            float* grad_rot_or_null, int B, int kind, int scale_h, double in_sz, double out_sz, void* stream) {
  using namespace hdn;
  if (!nm_shift || !scale || !rot || !grad) return HDN_E_NULL;
  if (const int rc = simi_geo::check_affine(B, kind, in_sz, out_sz, cx_or_null, cy_or_null)) return rc;
  if (!grad_nm_shift_or_null && !grad_scale_or_null && !grad_rot_or_null) return HDN_E_SHAPE;
  hipLaunchKernelGGL(simi_geo::affine_bwd_kernel, dim3(cdiv(B, HDN_BLOCK)), dim3(HDN_BLOCK), 0, static_cast<hipStream_t>(stream), nm_shift, scale, rot,
                     cx_or_null, cy_or_null, grad, grad_nm_shift_or_null, grad_scale_or_null, grad_rot_or_null, B, kind,
                     simi_geo::make_cfg(kind, cx_scalar, cy_scalar, scale_h, in_sz, out_sz));
  return launch_status();
}

int hdn_simi_warps_f32(const float* cls_lp, const float* loc_lp, const float* polar, const float* temp_cx, const float* temp_cy,
                       const float* search_poly, int* best_idx, float* scale, float* rot, float* affine_m, float* affine_m_lt0, float* affine_m_c_aug,
                       float* affine_m_lt0_aug, float* pred_points, float* aug_sear_points, int B, int S, int cls_channels, int stride, float stride_lp,
                       double mag, double rot_unit, double in_sz, double out_sz, void* stream) {
  using namespace hdn;
  if (!cls_lp || !loc_lp || !polar || !temp_cx || !temp_cy || !search_poly || !best_idx || !scale || !rot || !affine_m || !affine_m_lt0 ||
      !affine_m_c_aug || !affine_m_lt0_aug || !pred_points || !aug_sear_points)
    return HDN_E_NULL;
  if (cls_channels != 2 || !(in_sz > 0) || !(out_sz > 0)) return HDN_E_SHAPE;
  if (const int rc = simi_geo::check_pick(B, S, stride)) return rc;
  hipLaunchKernelGGL(simi_geo::warps_kernel, dim3(B), dim3(HDN_WAVE), 0, static_cast<hipStream_t>(stream), cls_lp, loc_lp, polar, temp_cx, temp_cy,
                     search_poly, best_idx, scale, rot, affine_m, affine_m_lt0, affine_m_c_aug, affine_m_lt0_aug, pred_points, aug_sear_points, S,
                     stride, stride_lp, (float)mag, (float)rot_unit, simi_geo::make_cfg(0, out_sz / 2, out_sz / 2, 1, in_sz, out_sz),
                     simi_geo::make_cfg(1, out_sz / 2, out_sz / 2, 1, in_sz, out_sz));
  return launch_status();
}

int hdn_simi_warps_bwd_f32(const int* best_idx, const float* scale, const float* rot, const float* polar, const float* search_poly,
                           const float* grad_scale_or_null, const float* grad_rot_or_null, const float* grad_affine_m_or_null,
                           const float* grad_affine_m_lt0_or_null, const float* grad_pred_points_or_null, float* grad_loc_lp_or_null,
                           float* grad_polar_or_null, int B, int S, float stride_lp, double mag, double rot_unit, double in_sz, double out_sz,
                           void* stream) {
  using namespace hdn;
  if (!best_idx || !scale || !rot || !polar || !search_poly) return HDN_E_NULL;
  if (!(in_sz > 0) || !(out_sz > 0) || (!grad_loc_lp_or_null && !grad_polar_or_null)) return HDN_E_SHAPE;
  if (const int rc = simi_geo::check_pick(B, S, 1)) return rc;
  hipLaunchKernelGGL(simi_geo::warps_bwd_kernel, dim3(B), dim3(HDN_WAVE), 0, static_cast<hipStream_t>(stream), best_idx, scale, rot, polar,
                     search_poly, grad_scale_or_null, grad_rot_or_null, grad_affine_m_or_null, grad_affine_m_lt0_or_null, grad_pred_points_or_null,
                     grad_loc_lp_or_null, grad_polar_or_null, S, stride_lp, (float)mag, (float)rot_unit,
                     simi_geo::make_cfg(0, out_sz / 2, out_sz / 2, 1, in_sz, out_sz), simi_geo::make_cfg(1, out_sz / 2, out_sz / 2, 1, in_sz, out_sz));
  return launch_status();
}

}  // extern "C"
