// The corner supervision of the similarity model's training forward (model_builder_e2e_unconstrained_v2.py:441-444, :481-523, :552-556), forward and
// backward, for gfx950:
//
//   hdn_corner_losses_f32       out[6] = cor_err, cor_err_aug, cor_err_sim, cor_pos_loss, cor_neg_loss, cor_loss and counts[6]
//   hdn_corner_losses_bwd_f32   the gradients of H_mat, pred_points, aug_sear_points and x for grad_out[6]
//
// The formulas are in include/hdn_hip.h.  A sample owns an aligned group of eight lanes, lane r = 2 j + c holding coordinate c of corner j (the
// order of template_poly, x and delta), so the 8 x 8 DLT system of cor_pos_loss is solved by dlt_row + solve8 of geometry.h in the group's
// registers, in float64, as hdn_dlt_solve_f32 solves it.  The six sample sets are decided from the flags in the kernel (set_flags): nothing is
// read by the host, nothing is uploaded.
//
// Forward: ONE workgroup of 1024 threads walks the batch 128 samples at a time.  A lane adds its terms in ascending sample order, the workgroup adds its
// lanes in the fixed order of reduce.h (block_sum_store): no float atomics, every output has the same bits on every call.  Backward: 32 samples per workgroup; each workgroup recounts the sets (integers: no order), then a row depends on its own sample
// and on the counts alone.
//
// A sample outside a set is never loaded for that set's terms: its lanes compute on a stand-in (H = I, the corners of the 127-square,
// w = 1, off = 0: a regular system) and the result is dropped by a select, never by a multiplication, so a NaN or a collinear polygon in such a
// sample reaches nothing.  Bounds: every index is b 8 + r, b 9 + q or b 12 + q with b < B <= MAX_B.
#include "geometry.h"

#pragma clang fp contract(off)

namespace hdn {
namespace corner {

constexpr int FWD_BLOCK = 1024;
constexpr int FWD_WAVES = FWD_BLOCK / HDN_WAVE;
constexpr int MAX_B = 1 << 16;
enum { N_SUP, N_SUP_POS, N_SUP_NEG, N_UNSUP, N_UNSUP_POS, N_NEG, N_SETS };

// the reference's predicates: float comparisons with 0 and 1 (.eq()); a flag that is neither fails them all
struct Sets {
  bool in[N_SETS];
};
__device__ __forceinline__ Sets set_flags(float pos, float un, bool valid) {
  Sets s;
  s.in[N_SUP] = valid && un == 0.f;
  s.in[N_SUP_POS] = valid && un == 0.f && pos == 1.f;
  s.in[N_SUP_NEG] = valid && un == 0.f && pos == 0.f;
  s.in[N_UNSUP] = valid && un == 1.f;
  s.in[N_UNSUP_POS] = valid && rn_mul(pos, un) == 1.f;  // (if_pos * if_unsup).eq(1)
  s.in[N_NEG] = valid && pos == 0.f;
  return s;
}

// coordinate r = 2 j + c of [[0,0],[0,127],[127,127],[127,0]]
__device__ __forceinline__ float square_coord(int r) {
  const int j = r >> 1;
  return (r & 1) ? ((j == 1 || j == 2) ? 127.f : 0.f) : (j >= 2 ? 127.f : 0.f);
}

__device__ __forceinline__ float sign_of(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }  // torch.sign: 0 at 0 (and at NaN)

// one element of kalyo_l1_loss (loss.py:201, norm=False) and its derivative in d; |d| = 1 belongs to the linear branch
__device__ __forceinline__ float kalyo_elem(float d) {
  const float a = fabsf(d);
  return a < 1.f ? rn_mul(0.5f, rn_mul(d, d)) : rn_sub(a, 0.5f);
}
__device__ __forceinline__ float kalyo_slope(float d) { return fabsf(d) < 1.f ? d : sign_of(d); }

// What lane r of a sample holds: its inputs (the stand-in where the sample is in no set that reads them) and the forward values both kernels need.
struct Lane {
  float t;                    // template_poly[b][j][c]
  float px, py, pw, pc;       // pred_points[b][:, j]; pc = row c
  float Hc[3], Hw[3];         // H_mat[b] rows c and 2
  float Pw, cor;              // (H P)_w and (H P)_c / (H P)_w
  float homo;                 // pc / pw
  float Qw, q, delta;         // H_gt applied to corner j: Q_w, Q_c / Q_w, and minus the corner
  double h;                   // the r-th unknown of the solve, before its rounding to fp32
};

// src_s / off_s: the group's eight floats in LDS (dlt_row reads through pointers).  Every thread of the block calls it.
__device__ __forceinline__ Lane lane_forward(const float* __restrict__ H, const float* __restrict__ pp, const float* __restrict__ tp, int b, int r,
                                             bool sup_pos, bool points, float* src_s, float* off_s) {
  Lane L;
  const int j = r >> 1, c = r & 1;
  const float sq = square_coord(r);
  L.t = points ? tp[size_t(b) * 8 + r] : sq;
  L.px = points ? pp[size_t(b) * 12 + j] : square_coord(2 * j);
  L.py = points ? pp[size_t(b) * 12 + 4 + j] : square_coord(2 * j + 1);
  L.pw = points ? pp[size_t(b) * 12 + 8 + j] : 1.f;
  L.pc = c ? L.py : L.px;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    L.Hc[k] = sup_pos ? H[size_t(b) * 9 + 3 * c + k] : (k == c ? 1.f : 0.f);
    L.Hw[k] = sup_pos ? H[size_t(b) * 9 + 6 + k] : (k == 2 ? 1.f : 0.f);
  }
  // torch.bmm(H_mat, pred_points), then the division by its w row (:485-486)
  const float Pc = rn_add(rn_add(rn_mul(L.Hc[0], L.px), rn_mul(L.Hc[1], L.py)), rn_mul(L.Hc[2], L.pw));
  L.Pw = rn_add(rn_add(rn_mul(L.Hw[0], L.px), rn_mul(L.Hw[1], L.py)), rn_mul(L.Hw[2], L.pw));
  L.cor = rn_div(Pc, L.Pw);
  // H_gt = DLT(template_poly, pred_points_xy / pred_points_w - template_poly) (:500-502), the system and elimination of hdn_dlt_solve_f32
  L.homo = rn_div(L.pc, L.pw);
  const int base = threadIdx.x & ~7;
  src_s[threadIdx.x] = sup_pos ? L.t : sq;
  off_s[threadIdx.x] = sup_pos ? rn_sub(L.homo, L.t) : 0.f;
  __syncthreads();
  L.h = solve8(dlt_row(src_s + base, off_s + base, r), r);
  float h[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) h[k] = __shfl((float)L.h, k, 8);
  // Q = H_gt [c_j; 1], delta = Q_xy / Q_w - c_j (:509-514)
  const float cx = square_coord(2 * j), cy = square_coord(2 * j + 1);
  const float Qc = rn_add(rn_add(rn_mul(c ? h[3] : h[0], cx), rn_mul(c ? h[4] : h[1], cy)), c ? h[5] : h[2]);
  L.Qw = rn_add(rn_add(rn_mul(h[6], cx), rn_mul(h[7], cy)), 1.f);
  L.q = rn_div(Qc, L.Qw);
  L.delta = rn_sub(L.q, sq);
  return L;
}

// v summed over the four corners of a sample (the lanes of equal c): the same bits in each of them
__device__ __forceinline__ float sum_corners(float v) {
  v = rn_add(v, __shfl_xor(v, 2, 8));
  return rn_add(v, __shfl_xor(v, 4, 8));
}

__global__ __launch_bounds__(FWD_BLOCK) void fwd_kernel(const float* __restrict__ H, const float* __restrict__ pp, const float* __restrict__ aug,
                                                        const float* __restrict__ tp, const float* __restrict__ x,
                                                        const float* __restrict__ if_pos, const float* __restrict__ if_unsup,
                                                        float* __restrict__ out, int* __restrict__ counts, int B) {
  __shared__ float src_s[FWD_BLOCK], off_s[FWD_BLOCK];
  __shared__ float red_f[FWD_WAVES * 5];
  __shared__ int red_i[FWD_WAVES * N_SETS];
  __shared__ float tot_f[5];
  __shared__ int tot_i[N_SETS];
  const int tid = threadIdx.x, r = tid & 7, j = r >> 1, c = r & 1;
  float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};  // the sums of slots 0 .. 4
  int cnt[N_SETS] = {0, 0, 0, 0, 0, 0};
  for (int first = 0; first < B; first += FWD_BLOCK / 8) {  // block-uniform: every thread meets the barriers of lane_forward
    const int g = first + (tid >> 3);
    const bool valid = g < B;
    const int b = valid ? g : B - 1;
    const Sets s = set_flags(if_pos[b], if_unsup[b], valid);
    const bool sp = s.in[N_SUP_POS], up = s.in[N_UNSUP_POS], ng = s.in[N_NEG];
    const Lane L = lane_forward(H, pp, tp, b, r, sp, sp || up, src_s, off_s);
    __syncthreads();  // the next round writes src_s / off_s
    const float xv = (sp || ng) ? x[size_t(b) * 8 + r] : 0.f;
    const float av = (sp && aug) ? aug[size_t(b) * 12 + 4 * c + j] : L.t;
    if (sp) {
      acc[0] = rn_add(acc[0], fabsf(rn_sub(L.cor, L.t)));
      acc[1] = rn_add(acc[1], fabsf(rn_sub(av, L.t)));
      acc[3] = rn_add(acc[3], kalyo_elem(rn_sub(L.delta, xv)));
    }
    if (up) acc[2] = rn_add(acc[2], fabsf(rn_sub(L.pc, L.t)));
    if (ng) acc[4] = rn_add(acc[4], kalyo_elem(rn_sub(0.f, xv)));
    if (r == 0) {
#pragma unroll
      for (int q = 0; q < N_SETS; ++q) cnt[q] += s.in[q] ? 1 : 0;
    }
  }
  block_sum_store<5, FWD_WAVES>(acc, red_f, tot_f);
  block_sum_store<N_SETS, FWD_WAVES>(cnt, red_i, tot_i);
  __syncthreads();
  if (tid < N_SETS) counts[tid] = tot_i[tid];
  if (tid != 0) return;
  const int n_sp = tot_i[N_SUP_POS], n_sn = tot_i[N_SUP_NEG], n_up = tot_i[N_UNSUP_POS], n_ng = tot_i[N_NEG];
  out[0] = n_sp > 0 ? rn_div(rn_div(tot_f[0], (float)n_sp), 4.f) : 0.f;
  out[1] = n_sp > 0 ? rn_div(rn_div(tot_f[1], (float)n_sp), 4.f) : 0.f;
  out[2] = n_up > 0 ? rn_div(rn_div(tot_f[2], (float)n_up), 4.f) : 0.f;
  const float pos_loss = n_sp > 0 ? rn_div(tot_f[3], (float)(8 * n_sp + 1)) : 0.f;
  const float neg_loss = n_sn > 0 ? rn_div(tot_f[4], (float)(8 * n_ng + 1)) : 0.f;  // over every neg sample, reported with a supervised one (:519-523, :554)
  out[3] = pos_loss;
  out[4] = neg_loss;
  out[5] = rn_add(pos_loss, neg_loss);
}

__global__ __launch_bounds__(HDN_BLOCK) void bwd_kernel(const float* __restrict__ H, const float* __restrict__ pp, const float* __restrict__ aug,
                                                        const float* __restrict__ tp, const float* __restrict__ x,
                                                        const float* __restrict__ if_pos, const float* __restrict__ if_unsup,
                                                        const float* __restrict__ gout, float* __restrict__ gH, float* __restrict__ gpp,
                                                        float* __restrict__ gaug, float* __restrict__ gx, int B) {
  __shared__ float src_s[HDN_BLOCK], off_s[HDN_BLOCK];
  __shared__ int red_i[BLOCK_WAVES * 4];
  const int tid = threadIdx.x, r = tid & 7, j = r >> 1, c = r & 1;
  // the counts, as the forward found them
  int n[4] = {0, 0, 0, 0};  // sup_pos, sup_neg, unsup_pos, neg
  for (int i = tid; i < B; i += HDN_BLOCK) {
    const Sets s = set_flags(if_pos[i], if_unsup[i], true);
    n[0] += s.in[N_SUP_POS], n[1] += s.in[N_SUP_NEG], n[2] += s.in[N_UNSUP_POS], n[3] += s.in[N_NEG];
  }
  block_sum<BLOCK_WAVES>(n, red_i);
  // d L / d (the five sums): out = (S / n) / 4 and S / tsz; cor_loss adds slot 3, and slot 4 where it is reported
  const float k0 = n[0] > 0 ? rn_div(rn_div(gout[0], 4.f), (float)n[0]) : 0.f;
  const float k1 = n[0] > 0 ? rn_div(rn_div(gout[1], 4.f), (float)n[0]) : 0.f;
  const float k2 = n[2] > 0 ? rn_div(rn_div(gout[2], 4.f), (float)n[2]) : 0.f;
  const float k3 = n[0] > 0 ? rn_div(rn_add(gout[3], gout[5]), (float)(8 * n[0] + 1)) : 0.f;
  const float k4 = n[1] > 0 ? rn_div(rn_add(gout[4], gout[5]), (float)(8 * n[3] + 1)) : 0.f;

  const int g = blockIdx.x * (HDN_BLOCK / 8) + (tid >> 3);
  const bool valid = g < B;
  const int b = valid ? g : B - 1;
  const Sets s = set_flags(if_pos[b], if_unsup[b], valid);
  const bool sp = s.in[N_SUP_POS], up = s.in[N_UNSUP_POS], ng = s.in[N_NEG];
  const Lane L = lane_forward(H, pp, tp, b, r, sp, sp || up, src_s, off_s);
  const float xv = (sp || ng) ? x[size_t(b) * 8 + r] : 0.f;
  const float av = (sp && aug) ? aug[size_t(b) * 12 + 4 * c + j] : L.t;
  const float* src = src_s + (tid & ~7);
  const float* off = off_s + (tid & ~7);

  // ---- cor_pos_loss: delta = Q_c / Q_w - c_j, Q = H_gt [c_j; 1]
  const float gdelta = rn_mul(k3, kalyo_slope(rn_sub(L.delta, xv)));
  const float dQc = rn_div(gdelta, L.Qw);
  float dQw = -rn_div(rn_mul(gdelta, L.q), L.Qw);
  dQw = rn_add(dQw, __shfl_xor(dQw, 1, 8));
  const float cx = square_coord(2 * j), cy = square_coord(2 * j + 1);
  const float v0 = sum_corners(rn_mul(dQc, cx)), v1 = sum_corners(rn_mul(dQc, cy)), v2 = sum_corners(dQc);   // grad of H_gt's row c
  const float w0 = sum_corners(rn_mul(dQw, cx)), w1 = sum_corners(rn_mul(dQw, cy));                           // and of its row 2 (H_gt[8] is constant)
  const float a0 = __shfl(v0, 0, 8), a1 = __shfl(v1, 0, 8), a2 = __shfl(v2, 0, 8);
  const float b0 = __shfl(v0, 1, 8), b1 = __shfl(v1, 1, 8), b2 = __shfl(v2, 1, 8);
  const float gh = r == 0 ? a0 : r == 1 ? a1 : r == 2 ? a2 : r == 3 ? b0 : r == 4 ? b1 : r == 5 ? b2 : r == 6 ? w0 : w1;
  // the adjoint solve of dlt_solve_bwd_kernel (geometry_bwd.hip): A^T lambda = grad_h, grad_b = lambda, grad_A = -lambda h^T; grad_off only
  Row9 at;
#pragma unroll
  for (int q = 0; q < 8; ++q) at.v[q] = dlt_elem(src, off, q, r);
  at.v[8] = (double)gh;
  const double lam = solve8(at, r);
  const double h6 = __shfl(L.h, 6, 8), h7 = __shfl(L.h, 7, 8);
  const int p = dlt_point(j);
  const double goff_d = lam + lam * h6 * (double)src[2 * p] + lam * h7 * (double)src[2 * p + 1];  // lane r holds the gradient of off[2 p + c]
  const float goff = __shfl((float)goff_d, 2 * p + c, 8);                                           // dlt_point is an involution: now of off[r]
  // off = pc / pw - t
  const float s3c = rn_div(goff, L.pw);
  float s3w = -rn_div(rn_mul(goff, L.homo), L.pw);
  s3w = rn_add(s3w, __shfl_xor(s3w, 1, 8));

  // ---- cor_err: |P_c / P_w - t|, P = H_mat pred_points
  const float ge = rn_mul(k0, sign_of(rn_sub(L.cor, L.t)));
  const float dPc = rn_div(ge, L.Pw);
  float dPw = -rn_div(rn_mul(ge, L.cor), L.Pw);
  dPw = rn_add(dPw, __shfl_xor(dPw, 1, 8));
  const float dPo = __shfl_xor(dPc, 1, 8);  // the corner's other coordinate
  const float d0 = c ? dPo : dPc, d1 = c ? dPc : dPo;
  float gHc[3], gHw[3];
  const float pk[3] = {L.px, L.py, L.pw};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    gHc[k] = sum_corners(rn_mul(dPc, pk[k]));
    gHw[k] = sum_corners(rn_mul(dPw, pk[k]));
  }
  const float Ho0 = __shfl_xor(L.Hc[0], 1, 8), Ho1 = __shfl_xor(L.Hc[1], 1, 8), Ho2 = __shfl_xor(L.Hc[2], 1, 8);  // the other row of H_mat
  const float H0c = c ? Ho1 : L.Hc[0], H1c = c ? L.Hc[1] : Ho0;                                                   // H[0][c], H[1][c]
  const float H02 = c ? Ho2 : L.Hc[2], H12 = c ? L.Hc[2] : Ho2;                                                   // H[0][2], H[1][2]
  const float e0c = rn_add(rn_add(rn_mul(H0c, d0), rn_mul(H1c, d1)), rn_mul(c ? L.Hw[1] : L.Hw[0], dPw));
  const float e0w = rn_add(rn_add(rn_mul(H02, d0), rn_mul(H12, d1)), rn_mul(L.Hw[2], dPw));

  if (!valid) return;  // no shuffle below
  if (gx) gx[size_t(b) * 8 + r] = sp ? -gdelta : (ng ? -rn_mul(k4, kalyo_slope(rn_sub(0.f, xv))) : 0.f);
  if (gaug) {
    gaug[size_t(b) * 12 + 4 * c + j] = sp ? rn_mul(k1, sign_of(rn_sub(av, L.t))) : 0.f;
    if (c == 0) gaug[size_t(b) * 12 + 8 + j] = 0.f;
  }
  if (gpp) {
    gpp[size_t(b) * 12 + 4 * c + j] = sp ? rn_add(e0c, s3c) : (up ? rn_mul(k2, sign_of(rn_sub(L.pc, L.t))) : 0.f);
    if (c == 0) gpp[size_t(b) * 12 + 8 + j] = sp ? rn_add(e0w, s3w) : 0.f;
  }
  if (gH) {
    if (j == 0)
      for (int k = 0; k < 3; ++k) gH[size_t(b) * 9 + 3 * c + k] = sp ? gHc[k] : 0.f;
    if (r == 2)
      for (int k = 0; k < 3; ++k) gH[size_t(b) * 9 + 6 + k] = sp ? gHw[k] : 0.f;
  }
}

}  // namespace corner
}  // namespace hdn

extern "C" {

int hdn_corner_losses_f32(const float* H_mat, const float* pred_points, const float* aug_sear_points_or_null, const float* template_poly,
                          const float* x, const float* if_pos, const float* if_unsup, float* out, int* counts, int B, void* stream) {
  using namespace hdn;
  if (!H_mat || !pred_points || !template_poly || !x || !if_pos || !if_unsup || !out || !counts) return HDN_E_NULL;
  if (B < 1) return HDN_E_SHAPE;
  if (B > corner::MAX_B) return HDN_E_LIMIT;
  hipLaunchKernelGGL(corner::fwd_kernel, dim3(1), dim3(corner::FWD_BLOCK), 0, static_cast<hipStream_t>(stream), H_mat, pred_points,
                     aug_sear_points_or_null, template_poly, x, if_pos, if_unsup, out, counts, B);
  return launch_status();
}

int hdn_corner_losses_bwd_f32(const float* H_mat, const float* pred_points, const float* aug_sear_points_or_null, const float* template_poly,
                              const float* x, const float* if_pos, const float* if_unsup, const float* grad_out, float* grad_H_mat_or_null,
                              float* grad_pred_points_or_null, float* grad_aug_sear_points_or_null, float* grad_x_or_null, int B, void* stream) {
  using namespace hdn;
  if (!H_mat || !pred_points || !template_poly || !x || !if_pos || !if_unsup || !grad_out) return HDN_E_NULL;
  if (grad_aug_sear_points_or_null && !aug_sear_points_or_null) return HDN_E_NULL;
  if (B < 1 || (!grad_H_mat_or_null && !grad_pred_points_or_null && !grad_aug_sear_points_or_null && !grad_x_or_null)) return HDN_E_SHAPE;
  if (B > corner::MAX_B) return HDN_E_LIMIT;
  hipLaunchKernelGGL(corner::bwd_kernel, dim3(cdiv(B, HDN_BLOCK / 8)), dim3(HDN_BLOCK), 0, static_cast<hipStream_t>(stream), H_mat, pred_points,
                     aug_sear_points_or_null, template_poly, x, if_pos, if_unsup, grad_out, grad_H_mat_or_null, grad_pred_points_or_null,
                     grad_aug_sear_points_or_null, grad_x_or_null, B);
  return launch_status();
}

}  // extern "C"
