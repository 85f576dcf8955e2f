// L1 triplet margin loss over rows for gfx950, forward and backward: hdn_triplet_l1_f32, hdn_triplet_l1_bwd_f32.  The formulas are in
// include/hdn_hip.h.  Reference: nn.TripletMarginLoss(margin=1.0, p=1, reduce=False, size_average=False) on three [n,1,127,127] ShareFeature maps
// that were gathered by x[ids] just before (model_builder_e2e_unconstrained_v2.py:438, homo_model_builder.py:197): F.pairwise_distance adds eps to the
// difference inside the absolute value, the loss is clamp_min((margin + d_ap) - d_an, 0).
//
// One wave per row, HDN_BLOCK / HDN_WAVE = 4 rows per workgroup.  A row of the reference is 127 floats and only 4-byte aligned, so lane l reads the
// dwords l, l + 64, ... of the three rows (coalesced, no wider access anywhere) and the two distances are reduced by wave_sum of reduce.h, which
// leaves the same sum in every lane.  The call is three reads of a 2 MB tensor at B = 32: launch and latency, not bandwidth; 3048 waves at 24 x 127 rows.
//
// The gather is folded into the addressing: with `ids`, row r of the result is row r % R of sample ids[r / R]; no gathered copy exists.  The sample
// index is checked against [0, N) before any address is formed: an index outside gives NaN loss rows and takes no part in the backward.
//
// The backward walks the full-size gradient rows (one wave per row of [N,R,D]): the wave looks its sample up in `ids` (lanes scan the list in strides
// of 64, the lowest matching position wins: ids are unique by contract, and a repeated one would otherwise be a race), recomputes v with row_v() - the
// forward's own function, so the decision v >= 0 is made on the forward's bits - and writes g sgn(.) per element, or zeros for a row that is not
// selected or not active.  Every gradient element is written exactly once by one lane: no atomics, no zero-fill pass, bit-reproducible.
#include "hdn_common.h"
#include "reduce.h"

#pragma clang fp contract(off)

namespace hdn {
namespace triplet {

constexpr int ROWS = HDN_BLOCK / HDN_WAVE;  // rows per workgroup

// |(x - y) + eps|: the subtraction rounded, then the add, as the two fp32 elementwise kernels of F.pairwise_distance do
__device__ __forceinline__ float term(float x, float y, float eps) { return fabsf(rn_add(rn_sub(x, y), eps)); }

__device__ __forceinline__ float sgn(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }  // sgn(0) = 0; NaN -> 0

// v = (margin + d_ap) - d_an of one row, the same value in every lane of the wave.  Lane l adds the elements l, l + 64, ... in ascending order, then
// wave_sum (reduce.h) adds the 64 partial sums.  The forward and the backward both call it.
__device__ __forceinline__ float row_v(const float* __restrict__ a, const float* __restrict__ p, const float* __restrict__ n, int D, int lane,
                                       float margin, float eps) {
  float d_ap = 0.f, d_an = 0.f;
  for (int j = lane; j < D; j += HDN_WAVE) {
    const float av = a[j], pv = p[j], nv = n[j];
    d_ap = rn_add(d_ap, term(av, pv, eps));
    d_an = rn_add(d_an, term(av, nv, eps));
  }
  return rn_sub(rn_add(margin, wave_sum(d_ap)), wave_sum(d_an));
}

__global__ __launch_bounds__(HDN_BLOCK) void fwd_kernel(const float* __restrict__ a, const float* __restrict__ p, const float* __restrict__ n,
                                                        const long long* __restrict__ ids, float* __restrict__ loss, int N, int R, int D,
                                                        long long rows, float margin, float eps) {
  const int lane = threadIdx.x & (HDN_WAVE - 1);
  const long long row = (long long)blockIdx.x * ROWS + (threadIdx.x / HDN_WAVE);
  if (row >= rows) return;                                   // wave-uniform
  const long long k = row / R;
  const int rr = (int)(row - k * R);
  const long long s = ids ? ids[k] : k;
  float out = __builtin_nanf("");
  if (s >= 0 && s < N) {                                     // checked before any address is formed
    const size_t off = (size_t(s) * R + rr) * size_t(D);
    const float v = row_v(a + off, p + off, n + off, D, lane, margin, eps);
    out = v < 0.f ? 0.f : v;                                 // clamp_min: v >= 0 and NaN pass
  }
  if (lane == 0) loss[row] = out;
}

__global__ __launch_bounds__(HDN_BLOCK) void bwd_kernel(const float* __restrict__ a, const float* __restrict__ p, const float* __restrict__ n,
                                                        const long long* __restrict__ ids, const float* __restrict__ gl, float* __restrict__ ga,
                                                        float* __restrict__ gp, float* __restrict__ gn, int N, int R, int D, int n_ids,
                                                        float margin, float eps) {
  const int lane = threadIdx.x & (HDN_WAVE - 1);
  const long long row = (long long)blockIdx.x * ROWS + (threadIdx.x / HDN_WAVE);
  if (row >= (long long)N * R) return;                       // wave-uniform
  const long long s = row / R;
  const int rr = (int)(row - s * R);
  long long k = s;                                           // position of sample s in the result; -1: not selected
  if (ids) {
    k = -1;
    for (int base = 0; base < n_ids && k < 0; base += HDN_WAVE) {
      const int q = base + lane;
      const bool hit = q < n_ids && ids[q] == s;
      const unsigned long long m = __ballot(hit);
      if (m) k = base + (__ffsll((long long)m) - 1);
    }
  }
  const size_t off = size_t(row) * size_t(D);
  bool active = false;
  float g = 0.f;
  if (k >= 0) {
    active = row_v(a + off, p + off, n + off, D, lane, margin, eps) >= 0.f;   // clamp_min's rule: the gradient passes at exactly 0, not at NaN
    g = gl[size_t(k) * R + rr];
  }
  if (!active) {                                             // wave-uniform
    for (int j = lane; j < D; j += HDN_WAVE) {
      if (ga) ga[off + j] = 0.f;
      if (gp) gp[off + j] = 0.f;
      if (gn) gn[off + j] = 0.f;
    }
    return;
  }
  for (int j = lane; j < D; j += HDN_WAVE) {
    const float av = a[off + j];
    const float s_ap = sgn(rn_add(rn_sub(av, p[off + j]), eps)), s_an = sgn(rn_add(rn_sub(av, n[off + j]), eps));
    if (ga) ga[off + j] = rn_mul(g, rn_sub(s_ap, s_an));     // g {0, +-1, +-2}: exact
    if (gp) gp[off + j] = rn_mul(-g, s_ap);
    if (gn) gn[off + j] = rn_mul(g, s_an);
  }
}

static int check_dims(const long long* ids, int N, int R, int D, int n_ids) {
  if (N <= 0 || R <= 0 || D <= 0 || (ids && n_ids <= 0)) return HDN_E_SHAPE;
  return HDN_OK;
}

static bool over_limit(const long long* ids, int N, int R, int D, int n_ids) {
  return (long long)N * R > (1LL << 30) || (ids && (long long)n_ids * R > (1LL << 30)) || D > (1 << 20);
}

}  // namespace triplet
}  // namespace hdn

extern "C" {

int hdn_triplet_l1_f32(const float* anchor, const float* positive, const float* negative, const long long* ids_or_null, float* loss, int N, int R,
                       int D, int n_ids, float margin, float eps, void* stream) {
  using namespace hdn;
  if (!anchor || !positive || !negative || !loss) return HDN_E_NULL;
  if (triplet::check_dims(ids_or_null, N, R, D, n_ids)) return HDN_E_SHAPE;
  if (triplet::over_limit(ids_or_null, N, R, D, n_ids)) return HDN_E_LIMIT;
  const long long rows = (long long)(ids_or_null ? n_ids : N) * R, in_bytes = (long long)N * R * D * 4, out_bytes = rows * 4;
  for (const float* in : {anchor, positive, negative})
    if (bytes_overlap(loss, out_bytes, in, in_bytes)) return HDN_E_ALIAS;
  if (ids_or_null && bytes_overlap(loss, out_bytes, ids_or_null, (long long)n_ids * 8)) return HDN_E_ALIAS;
  hipLaunchKernelGGL(triplet::fwd_kernel, dim3((unsigned)((rows + triplet::ROWS - 1) / triplet::ROWS)), dim3(HDN_BLOCK), 0,
                     static_cast<hipStream_t>(stream), anchor, positive, negative, ids_or_null, loss, N, R, D, rows, margin, eps);
  return launch_status();
}

int hdn_triplet_l1_bwd_f32(const float* anchor, const float* positive, const float* negative, const long long* ids_or_null, const float* grad_loss,
                           float* grad_a_or_null, float* grad_p_or_null, float* grad_n_or_null, int N, int R, int D, int n_ids, float margin,
                           float eps, void* stream) {
  using namespace hdn;
  if (!anchor || !positive || !negative || !grad_loss) return HDN_E_NULL;
  if (triplet::check_dims(ids_or_null, N, R, D, n_ids) || (!grad_a_or_null && !grad_p_or_null && !grad_n_or_null)) return HDN_E_SHAPE;
  if (triplet::over_limit(ids_or_null, N, R, D, n_ids)) return HDN_E_LIMIT;
  const long long rows = (long long)N * R, in_bytes = rows * D * 4, gl_bytes = (long long)(ids_or_null ? n_ids : N) * R * 4;
  float* const outs[3] = {grad_a_or_null, grad_p_or_null, grad_n_or_null};
  for (int i = 0; i < 3; ++i) {
    if (!outs[i]) continue;
    for (const float* in : {anchor, positive, negative})
      if (bytes_overlap(outs[i], in_bytes, in, in_bytes)) return HDN_E_ALIAS;
    if (bytes_overlap(outs[i], in_bytes, grad_loss, gl_bytes)) return HDN_E_ALIAS;
    if (ids_or_null && bytes_overlap(outs[i], in_bytes, ids_or_null, (long long)n_ids * 8)) return HDN_E_ALIAS;
    for (int j = 0; j < i; ++j)
      if (outs[j] && bytes_overlap(outs[i], in_bytes, outs[j], in_bytes)) return HDN_E_ALIAS;
  }
  hipLaunchKernelGGL(triplet::bwd_kernel, dim3((unsigned)((rows + triplet::ROWS - 1) / triplet::ROWS)), dim3(HDN_BLOCK), 0,
                     static_cast<hipStream_t>(stream), anchor, positive, negative, ids_or_null, grad_loss, grad_a_or_null, grad_p_or_null,
                     grad_n_or_null, N, R, D, n_ids, margin, eps);
  return launch_status();
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------------------------------------
// The flag-selected mean of the rows above: hdn_triplet_l1_mean_f32, hdn_triplet_l1_mean_bwd_f32 (formulas: include/hdn_hip.h).  The two triplet terms
// of the training forwards (model_builder_e2e_unconstrained_v2.py:430-440, homo_model_builder.py:174-199) select their samples with nonzero() and
// divide by a length read on the host; here the sets are decided from if_pos / if_unsup in the kernels, so nothing is read by the host.
//
// Forward, two launches in one call.  rows: one wave per row of [N,R,D], as fwd_kernel; the row's clamped loss (row_v(), the bits of the kernels
// above) goes to partial[row], 0 for a row of a sample that is not used, whose data is not read.  finish: ONE workgroup of 1024 threads; thread t
// adds partial[t], partial[t + 1024], ... in ascending order, block_sum of reduce.h adds the threads: the order depends on (N, R) alone, no float atomics, no hand-off between workgroups inside a launch (the stream orders the two
// kernels).  Backward: one wave per gradient row, every element written exactly once.  Each workgroup counts the sets itself (integers: no order).
// Bounds: a flag index is < N, a row index < N R, an element index < N R D; partial has N R floats.
namespace hdn {
namespace triplet {

constexpr int MEAN_MAX_N = 1 << 16;
constexpr int FIN_BLOCK = 1024;

// the reference's predicates, float comparisons as .eq() makes them: a flag of 0.5 or NaN fails both
__device__ __forceinline__ bool is_sel(float pos, float un) { return rn_mul(pos, un) == 1.f; }  // (if_pos * if_unsup).eq(1)
__device__ __forceinline__ bool is_neg(float pos) { return pos == 0.f; }                        // if_pos.eq(0)

// is a sample read?  rule 0: the selected ones; rule 1: the selected ones where the batch has a negative, every sample otherwise; none while n_sel = 0
__device__ __forceinline__ bool sample_used(bool sel, int rule, int n_sel, int n_neg) { return n_sel > 0 && (sel || (rule == 1 && n_neg == 0)); }

// n_sel and n_neg of the batch, the same in every thread.  Every thread of the workgroup calls it (block_sum's barriers); red: 2 BLOCK / 64 ints of LDS.
template <int BLOCK>
__device__ __forceinline__ void count_sets(const float* __restrict__ if_pos, const float* __restrict__ if_unsup, int N, int* red, int& n_sel,
                                           int& n_neg) {
  int c[2] = {0, 0};
  for (int i = threadIdx.x; i < N; i += BLOCK) {
    const float pos = if_pos[i];
    c[0] += is_sel(pos, if_unsup[i]) ? 1 : 0;
    c[1] += is_neg(pos) ? 1 : 0;
  }
  block_sum<BLOCK / HDN_WAVE>(c, red);
  n_sel = c[0], n_neg = c[1];
}

__global__ __launch_bounds__(HDN_BLOCK) void mean_rows_kernel(const float* __restrict__ a, const float* __restrict__ p, const float* __restrict__ n,
                                                              const float* __restrict__ if_pos, const float* __restrict__ if_unsup,
                                                              float* __restrict__ partial, int N, int R, int D, int rule, float margin, float eps) {
  __shared__ int red[2 * ROWS];
  int n_sel = 1, n_neg = 1;                                    // rule 0 asks for neither: a selected sample is used
  if (rule == 1) count_sets<HDN_BLOCK>(if_pos, if_unsup, N, red, n_sel, n_neg);   // uniform over the launch: every thread meets the barrier
  const int lane = threadIdx.x & (HDN_WAVE - 1);
  const long long row = (long long)blockIdx.x * ROWS + (threadIdx.x / HDN_WAVE);
  if (row >= (long long)N * R) return;                         // wave-uniform, after the barrier
  const int s = (int)(row / R);
  float out = 0.f;
  if (sample_used(is_sel(if_pos[s], if_unsup[s]), rule, n_sel, n_neg)) {   // wave-uniform; nothing of an unused sample is read
    const size_t off = size_t(row) * size_t(D);
    const float v = row_v(a + off, p + off, n + off, D, lane, margin, eps);
    out = v < 0.f ? 0.f : v;                                   // clamp_min: v >= 0 and NaN pass
  }
  if (lane == 0) partial[row] = out;
}

__global__ __launch_bounds__(FIN_BLOCK) void mean_finish_kernel(const float* __restrict__ partial, const float* __restrict__ if_pos,
                                                                const float* __restrict__ if_unsup, float* __restrict__ out,
                                                                int* __restrict__ counts, int N, long long rows, int rule, float denom) {
  __shared__ int red[2 * (FIN_BLOCK / HDN_WAVE)];
  __shared__ float red_f[FIN_BLOCK / HDN_WAVE];
  int n_sel, n_neg;
  count_sets<FIN_BLOCK>(if_pos, if_unsup, N, red, n_sel, n_neg);
  float acc = 0.f;
  for (long long i = threadIdx.x; i < rows; i += FIN_BLOCK) acc = rn_add(acc, partial[i]);
  const float S = block_sum<FIN_BLOCK / HDN_WAVE>(acc, red_f);
  if (threadIdx.x != 0) return;
  const float ns = (float)n_sel;
  out[0] = n_sel > 0 ? (rule == 0 ? rn_div(rn_div(S, denom), ns) : rn_div(rn_div(S, ns), denom)) : 0.f;
  counts[0] = n_sel;
  counts[1] = n_neg;
}

__global__ __launch_bounds__(HDN_BLOCK) void mean_bwd_kernel(const float* __restrict__ a, const float* __restrict__ p, const float* __restrict__ n,
                                                             const float* __restrict__ if_pos, const float* __restrict__ if_unsup,
                                                             const float* __restrict__ gout, float* __restrict__ ga, float* __restrict__ gp,
                                                             float* __restrict__ gn, int N, int R, int D, int rule, float denom, float margin,
                                                             float eps) {
  __shared__ int red[2 * ROWS];
  int n_sel, n_neg;
  count_sets<HDN_BLOCK>(if_pos, if_unsup, N, red, n_sel, n_neg);   // the sets as the forward found them
  const int lane = threadIdx.x & (HDN_WAVE - 1);
  const long long row = (long long)blockIdx.x * ROWS + (threadIdx.x / HDN_WAVE);
  if (row >= (long long)N * R) return;                         // wave-uniform, after the barrier
  const int s = (int)(row / R);
  const size_t off = size_t(row) * size_t(D);
  bool active = false;
  if (sample_used(is_sel(if_pos[s], if_unsup[s]), rule, n_sel, n_neg))
    active = row_v(a + off, p + off, n + off, D, lane, margin, eps) >= 0.f;   // clamp_min's rule, on the forward's bits
  if (!active) {                                               // wave-uniform
    for (int j = lane; j < D; j += HDN_WAVE) {
      if (ga) ga[off + j] = 0.f;
      if (gp) gp[off + j] = 0.f;
      if (gn) gn[off + j] = 0.f;
    }
    return;
  }
  const float g = gout[0], ns = (float)n_sel;                  // n_sel > 0: a sample is used
  const float c = rule == 0 ? rn_div(rn_div(g, denom), ns) : rn_div(rn_div(g, ns), denom);
  for (int j = lane; j < D; j += HDN_WAVE) {
    const float av = a[off + j];
    const float s_ap = sgn(rn_add(rn_sub(av, p[off + j]), eps)), s_an = sgn(rn_add(rn_sub(av, n[off + j]), eps));
    if (ga) ga[off + j] = rn_mul(c, rn_sub(s_ap, s_an));       // c {0, +-1, +-2}: exact
    if (gp) gp[off + j] = rn_mul(-c, s_ap);
    if (gn) gn[off + j] = rn_mul(c, s_an);
  }
}

static int mean_check_dims(int N, int R, int D, int rule, float denom) {
  if (N <= 0 || R <= 0 || D <= 0 || (rule != 0 && rule != 1) || !(denom > 0.f)) return HDN_E_SHAPE;
  return HDN_OK;
}

static bool mean_over_limit(int N, int R, int D) { return N > MEAN_MAX_N || (long long)N * R > (1LL << 30) || D > (1 << 20); }

}  // namespace triplet
}  // namespace hdn

extern "C" {

int hdn_triplet_l1_mean_f32(const float* anchor, const float* positive, const float* negative, const float* if_pos, const float* if_unsup,
                            float* partial, float* out, int* counts, int N, int R, int D, int rule, float denom, float margin, float eps,
                            void* stream) {
  using namespace hdn;
  if (!anchor || !positive || !negative || !if_pos || !if_unsup || !partial || !out || !counts) return HDN_E_NULL;
  if (triplet::mean_check_dims(N, R, D, rule, denom)) return HDN_E_SHAPE;
  if (triplet::mean_over_limit(N, R, D)) return HDN_E_LIMIT;
  const long long rows = (long long)N * R, in_bytes = rows * D * 4, flag_bytes = (long long)N * 4;
  const void* const outs[3] = {partial, out, counts};
  const long long out_bytes[3] = {rows * 4, 4, 8};
  for (int i = 0; i < 3; ++i) {
    for (const float* in : {anchor, positive, negative})
      if (bytes_overlap(outs[i], out_bytes[i], in, in_bytes)) return HDN_E_ALIAS;
    for (const float* in : {if_pos, if_unsup})
      if (bytes_overlap(outs[i], out_bytes[i], in, flag_bytes)) return HDN_E_ALIAS;
    for (int j = 0; j < i; ++j)
      if (bytes_overlap(outs[i], out_bytes[i], outs[j], out_bytes[j])) return HDN_E_ALIAS;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(triplet::mean_rows_kernel, dim3((unsigned)((rows + triplet::ROWS - 1) / triplet::ROWS)), dim3(HDN_BLOCK), 0, st, anchor,
                     positive, negative, if_pos, if_unsup, partial, N, R, D, rule, margin, eps);
  if (const int rc = launch_status()) return rc;
  hipLaunchKernelGGL(triplet::mean_finish_kernel, dim3(1), dim3(triplet::FIN_BLOCK), 0, st, partial, if_pos, if_unsup, out, counts, N, rows, rule,
                     denom);
  return launch_status();
}

int hdn_triplet_l1_mean_bwd_f32(const float* anchor, const float* positive, const float* negative, const float* if_pos, const float* if_unsup,
                                const float* grad_out, float* grad_a_or_null, float* grad_p_or_null, float* grad_n_or_null, int N, int R, int D,
                                int rule, float denom, float margin, float eps, void* stream) {
  using namespace hdn;
  if (!anchor || !positive || !negative || !if_pos || !if_unsup || !grad_out) return HDN_E_NULL;
  if (triplet::mean_check_dims(N, R, D, rule, denom) || (!grad_a_or_null && !grad_p_or_null && !grad_n_or_null)) return HDN_E_SHAPE;
  if (triplet::mean_over_limit(N, R, D)) return HDN_E_LIMIT;
  const long long rows = (long long)N * R, in_bytes = rows * D * 4, flag_bytes = (long long)N * 4;
  float* const outs[3] = {grad_a_or_null, grad_p_or_null, grad_n_or_null};
  for (int i = 0; i < 3; ++i) {
    if (!outs[i]) continue;
    for (const float* in : {anchor, positive, negative})
      if (bytes_overlap(outs[i], in_bytes, in, in_bytes)) return HDN_E_ALIAS;
    for (const float* in : {if_pos, if_unsup})
      if (bytes_overlap(outs[i], in_bytes, in, flag_bytes)) return HDN_E_ALIAS;
    if (bytes_overlap(outs[i], in_bytes, grad_out, 4)) return HDN_E_ALIAS;
    for (int j = 0; j < i; ++j)
      if (outs[j] && bytes_overlap(outs[i], in_bytes, outs[j], in_bytes)) return HDN_E_ALIAS;
  }
  hipLaunchKernelGGL(triplet::mean_bwd_kernel, dim3((unsigned)((rows + triplet::ROWS - 1) / triplet::ROWS)), dim3(HDN_BLOCK), 0,
                     static_cast<hipStream_t>(stream), anchor, positive, negative, if_pos, if_unsup, grad_out, grad_a_or_null, grad_p_or_null,
                     grad_n_or_null, N, R, D, rule, denom, margin, eps);
  return launch_status();
}

}  // extern "C"
