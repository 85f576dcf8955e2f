// The similarity model's supervised head losses for gfx950, forward and backward: hdn_sup_losses_f32, hdn_sup_losses_bwd_f32.  The formulas are in
// include/hdn_hip.h.  Reference: hdn/models/loss.py (select_xr_focal_fuse_smooth_l1_loss_top_k, select_l1_loss_c, select_cross_entropy_loss,
// select_l1_loss, kalyo_l1_loss) as model_builder_e2e_unconstrained_v2.py:457-478 and :516-523 call them: about a hundred elementwise, nonzero,
// index_select, topk and reduce launches forward, ten of them host synchronisations, over a few hundred kilobytes.
//
// One launch, one workgroup of T = 1024 threads per loss (blockIdx.x = loss; a loss whose pointers are NULL returns at once).  Everything the
// reference selects with nonzero() is a predicate here: the sample mask (if_unsup[b] == 0), the label tests, the label maximum of (b), the counts and
// the top-k of (a).  Thread t owns the cells t, t + T, ... and adds its terms in ascending order; the workgroup adds its threads with block_sum
// of reduce.h: the order is fixed, so every output is bit-reproducible.  No float atomics.
//
// Top-k of (a): l = -log(1 - p) is positive, so its bit pattern orders as its value.  The l of every negative cell is kept in LDS (4 bytes per cell,
// 0 for a cell that is no negative: at most MAX_CELLS = 40000 cells, 156.25 KiB, which is where the limit comes from), and the k-th largest is found
// by a radix select: four passes of 8 bits from the top, each an integer LDS histogram of the cells that match the digits found so far.  The sum of
// the k largest is sum{l > t} + (k - count_gt) t.  The backward repeats the selection (same device function, same bits), then ranks the cells equal to
// t by flat index over contiguous chunks and an exclusive scan, and keeps the lowest k - count_gt of them.
#include "hdn_common.h"
#include "reduce.h"

#pragma clang fp contract(off)

namespace hdn {
namespace sup {

constexpr int T = 1024;
constexpr int NW = T / HDN_WAVE;
constexpr int MAX_CELLS = 40000;             // B S^2 and B S_lp^2: 64 x 25 x 25; the LDS image of (a) is 4 bytes per cell
constexpr int MAX_ROW_ELEMS = 1 << 20;       // n_rows C of (e)
constexpr unsigned NAN_BITS = 0x7fc00000u;   // above every finite pattern and +inf: a NaN l is the largest, as in torch.topk

struct Scratch {
  float f[NW];
  int i[NW];
  unsigned hist[256];
  int pick[2];
};

// exclusive prefix sum of one int per thread, in thread order (a scan, not a reduction: it is not in reduce.h)
__device__ __forceinline__ int block_scan_exclusive(int v, Scratch& s) {
  const int lane = lane_id(), wave = wave_id();
  int inc = v;
#pragma unroll
  for (int d = 1; d < HDN_WAVE; d <<= 1) {
    const int o = __shfl_up(inc, d, HDN_WAVE);
    if (lane >= d) inc += o;
  }
  __syncthreads();
  if (lane == HDN_WAVE - 1) s.i[wave] = inc;
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wave; ++w) base += s.i[w];
  return base + inc - v;
}

__device__ __forceinline__ bool sample_on(const float* __restrict__ mask, int b) { return !mask || mask[b] == 0.f; }   // if_unsup.eq(0)

__device__ __forceinline__ int count_samples(const float* __restrict__ mask, int B, Scratch& s) {
  if (!mask) return B;
  int n = 0;
  for (int b = threadIdx.x; b < B; b += T) n += mask[b] == 0.f;
  return block_sum<NW>(n, s.i);
}

__device__ __forceinline__ float sgn(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }

// F.softmax over two logits as PyTorch evaluates it: exp(x - max) / sum
struct Soft2 {
  float p0, p1;
};
__device__ __forceinline__ Soft2 softmax2(float x0, float x1) {
  const float m = fmaxf(x0, x1);
  const float e0 = expf(rn_sub(x0, m)), e1 = expf(rn_sub(x1, m));
  const float sum = rn_add(e0, e1);
  return {rn_div(e0, sum), rn_div(e1, sum)};
}

// F.log_softmax over two logits: (x - max) - log(sum exp(x - max))
__device__ __forceinline__ Soft2 log_softmax2(float x0, float x1) {
  const float m = fmaxf(x0, x1);
  const float a0 = rn_sub(x0, m), a1 = rn_sub(x1, m);
  const float ls = logf(rn_add(expf(a0), expf(a1)));
  return {rn_sub(a0, ls), rn_sub(a1, ls)};
}

// the two class values of cell c of sample b.  form 0: raw maps [B,2,S,S]; form 1: [n,S,S,2]
__device__ __forceinline__ void load2(const float* __restrict__ x, int form, int b, int c, int S2, float& v0, float& v1) {
  if (form == 0) {
    v0 = x[(b * 2 + 0) * S2 + c];
    v1 = x[(b * 2 + 1) * S2 + c];
  } else {
    v0 = x[(b * S2 + c) * 2 + 0];
    v1 = x[(b * S2 + c) * 2 + 1];
  }
}

constexpr float CLAMP_LO = 0.000001f, CLAMP_HI = 0.9999999f;

__device__ __forceinline__ float clamp_p(float p) { return p != p ? p : fminf(fmaxf(p, CLAMP_LO), CLAMP_HI); }

__device__ __forceinline__ unsigned l_bits(float p1) {
  const float l = -logf(rn_sub(1.f, clamp_p(p1)));
  return l != l ? NAN_BITS : __float_as_uint(l);
}

// ------------------------------------------------------------------------------------------------------------------------------------------ (a)
struct SelA {
  int n_pos, k_eff, rem;      // rem: how many of the cells equal to t belong to the top k
  unsigned tbits;             // the k-th largest l (valid when k_eff > 0)
  float pos_sum, top_sum;     // sum |label - p1| over the positives; sum of the k largest l
};

// Everything (a) selects.  lb [cells] (LDS) receives the bits of l for every negative cell and 0 elsewhere.
__device__ SelA select_a(const float* __restrict__ cls, const float* __restrict__ label, const float* __restrict__ mask, int form, int B, int S2,
                         int topk, unsigned* lb, Scratch& s) {
  const int cells = B * S2, tid = threadIdx.x;
  const int n = count_samples(mask, B, s);
  float pos_sum = 0.f;
  int n_pos = 0, n_neg = 0;
  for (int i = tid; i < cells; i += T) {
    const int b = i / S2, c = i - b * S2;
    unsigned bits = 0;
    if (sample_on(mask, b)) {
      const float L = label[i];
      float v0, v1;
      load2(cls, form, b, c, S2, v0, v1);
      const float p1 = form == 0 ? softmax2(v0, v1).p1 : v1;
      if (L > 0.f) {
        pos_sum = rn_add(pos_sum, fabsf(rn_sub(L, p1)));
        ++n_pos;
      } else if (L == 0.f) {
        bits = l_bits(p1);
        ++n_neg;
      }
    }
    lb[i] = bits;
  }
  SelA r;
  r.n_pos = block_sum<NW>(n_pos, s.i);
  n_neg = block_sum<NW>(n_neg, s.i);
  r.pos_sum = block_sum<NW>(pos_sum, s.f);
  const long long k = (long long)topk * n;
  r.k_eff = n_neg <= 1 ? 0 : (int)(k < n_neg ? k : n_neg);     // one negative: the reference's 0-d index, the term is 0
  r.rem = 0;
  r.tbits = 0xffffffffu;
  r.top_sum = 0.f;
  if (r.k_eff == 0) return r;                                   // block-uniform
  unsigned prefix = 0;
  int rem = r.k_eff;
  for (int shift = 24; shift >= 0; shift -= 8) {
    __syncthreads();
    if (tid < 256) s.hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < cells; i += T) {
      const unsigned bits = lb[i];
      if (bits != 0 && (shift == 24 || (bits >> (shift + 8)) == (prefix >> (shift + 8)))) atomicAdd(&s.hist[(bits >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      int d = 255, left = rem;
      for (; d > 0; --d) {
        const int c = (int)s.hist[d];
        if (left <= c) break;
        left -= c;
      }
      s.pick[0] = d;
      s.pick[1] = left;
    }
    __syncthreads();
    prefix |= (unsigned)s.pick[0] << shift;
    rem = s.pick[1];
  }
  r.tbits = prefix;
  r.rem = rem;
  float acc = 0.f;
  for (int i = tid; i < cells; i += T) {
    const unsigned bits = lb[i];
    if (bits > prefix) acc = rn_add(acc, __uint_as_float(bits));
  }
  r.top_sum = rn_add(block_sum<NW>(acc, s.f), rn_mul((float)rem, __uint_as_float(prefix)));
  return r;
}

__device__ void fwd_a(const float* cls, const float* label, const float* mask, int form, int B, int S2, int topk, unsigned* lb, Scratch& s,
                      float* out) {
  const SelA r = select_a(cls, label, mask, form, B, S2, topk, lb, s);
  const float pos = r.n_pos <= 1 ? 0.f : rn_div(r.pos_sum, (float)(r.n_pos + 1));
  const float neg = r.k_eff == 0 ? 0.f : rn_div(r.top_sum, (float)(r.k_eff + 1));
  if (threadIdx.x == 0) *out = rn_add(pos, neg);
}

__device__ void bwd_a(const float* cls, const float* label, const float* mask, int form, int B, int S2, int topk, unsigned* lb, Scratch& s, float g,
                      float* __restrict__ grad) {
  const SelA r = select_a(cls, label, mask, form, B, S2, topk, lb, s);
  const int cells = B * S2, tid = threadIdx.x;
  __syncthreads();
  if (r.k_eff > 0) {
    // the cells equal to t, ranked by flat index: the lowest r.rem keep their bits, the others are struck out
    const int chunk = (cells + T - 1) / T, lo = min(tid * chunk, cells), hi = min(lo + chunk, cells);
    int ties = 0;
    for (int i = lo; i < hi; ++i) ties += lb[i] == r.tbits;
    int rank = block_scan_exclusive(ties, s);
    for (int i = lo; i < hi; ++i)
      if (lb[i] == r.tbits) {
        if (rank >= r.rem) lb[i] = 0;
        ++rank;
      }
    __syncthreads();
  }
  const float g_pos = r.n_pos <= 1 ? 0.f : rn_div(g, (float)(r.n_pos + 1));
  const float g_neg = r.k_eff == 0 ? 0.f : rn_div(g, (float)(r.k_eff + 1));
  for (int i = tid; i < cells; i += T) {
    const int b = i / S2, c = i - b * S2;
    float gp = 0.f, p0 = 0.f, p1 = 0.f;
    if (sample_on(mask, b)) {
      const float L = label[i];
      float v0, v1;
      load2(cls, form, b, c, S2, v0, v1);
      if (form == 0) {
        const Soft2 sm = softmax2(v0, v1);
        p0 = sm.p0, p1 = sm.p1;
      } else {
        p1 = v1;
      }
      if (L > 0.f) {
        gp = rn_mul(g_pos, sgn(rn_sub(p1, L)));
      } else if (L == 0.f && r.k_eff > 0 && lb[i] >= r.tbits && lb[i] != 0) {
        if (p1 >= CLAMP_LO && p1 <= CLAMP_HI) gp = rn_div(g_neg, rn_sub(1.f, p1));   // clamp passes the gradient on its closed interval
      }
    }
    if (form == 0) {
      const float gx1 = rn_mul(gp, rn_mul(p1, p0));        // d p1 / d x1 = p1 p0 = -d p1 / d x0
      grad[(b * 2 + 0) * S2 + c] = gp == 0.f ? 0.f : -gx1;
      grad[(b * 2 + 1) * S2 + c] = gp == 0.f ? 0.f : gx1;
    } else {
      grad[(b * S2 + c) * 2 + 0] = 0.f;
      grad[(b * S2 + c) * 2 + 1] = gp;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------------ (b), (d), (e)
// Smooth L1 over the selected cells of pred, target [B,C,S,S] (rows [n,C] are S = 1).  kind 0: every cell; 1: flabel > thr; 2: ilabel > 0.
__device__ __forceinline__ bool cell_on(int kind, const float* __restrict__ flabel, const long long* __restrict__ ilabel, float thr, int i) {
  return kind == 0 ? true : (kind == 1 ? flabel[i] > thr : ilabel[i] > 0);
}

// the threshold max_c - 0.2 of (b): max_c is the label maximum over the selected samples; a NaN label makes it NaN (torch.max), which selects nothing
__device__ float threshold_b(const float* __restrict__ flabel, const float* __restrict__ mask, int B, int S2, Scratch& s) {
  float m = -INFINITY;
  int nan = 0;
  for (int i = threadIdx.x; i < B * S2; i += T)
    if (sample_on(mask, i / S2)) {
      const float L = flabel[i];
      if (L != L) nan = 1; else m = fmaxf(m, L);
    }
  m = block_max<NW>(m, s.f);
  nan = block_sum<NW>(nan, s.i);
  return nan ? __builtin_nanf("") : rn_sub(m, 0.2f);
}

__device__ __forceinline__ float smooth_l1(float d) {
  const float ad = fabsf(d);
  return ad < 1.f ? rn_mul(0.5f, rn_mul(d, d)) : rn_sub(ad, 0.5f);
}

__device__ void fwd_smooth(const float* __restrict__ pred, const float* __restrict__ tgt, int kind, const float* flabel, const long long* ilabel,
                           const float* mask, int B, int C, int S2, bool one_hit_zero, Scratch& s, float* out) {
  const float thr = kind == 1 ? threshold_b(flabel, mask, B, S2, s) : 0.f;
  float acc = 0.f;
  int n_sel = 0;
  for (int i = threadIdx.x; i < B * S2; i += T) {
    const int b = i / S2, c = i - b * S2;
    if (!sample_on(mask, b) || !cell_on(kind, flabel, ilabel, thr, i)) continue;
    ++n_sel;
    for (int ch = 0; ch < C; ++ch) {
      const int idx = (b * C + ch) * S2 + c;
      acc = rn_add(acc, smooth_l1(rn_sub(pred[idx], tgt[idx])));
    }
  }
  n_sel = block_sum<NW>(n_sel, s.i);
  acc = block_sum<NW>(acc, s.f);
  if (threadIdx.x == 0) *out = (one_hit_zero && n_sel <= 1) ? 0.f : rn_div(acc, (float)(C * n_sel + 1));
}

__device__ void bwd_smooth(const float* __restrict__ pred, const float* __restrict__ tgt, int kind, const float* flabel, const long long* ilabel,
                           const float* mask, int B, int C, int S2, bool one_hit_zero, Scratch& s, float g, float* __restrict__ grad) {
  const float thr = kind == 1 ? threshold_b(flabel, mask, B, S2, s) : 0.f;
  int n_sel = 0;
  for (int i = threadIdx.x; i < B * S2; i += T) n_sel += sample_on(mask, i / S2) && cell_on(kind, flabel, ilabel, thr, i);
  n_sel = block_sum<NW>(n_sel, s.i);
  const float gs = (one_hit_zero && n_sel <= 1) ? 0.f : rn_div(g, (float)(C * n_sel + 1));
  for (int i = threadIdx.x; i < B * S2; i += T) {
    const int b = i / S2, c = i - b * S2;
    const bool on = gs != 0.f && sample_on(mask, b) && cell_on(kind, flabel, ilabel, thr, i);
    for (int ch = 0; ch < C; ++ch) {
      const int idx = (b * C + ch) * S2 + c;
      float v = 0.f;
      if (on) {
        const float d = rn_sub(pred[idx], tgt[idx]);
        v = rn_mul(gs, fabsf(d) < 1.f ? d : sgn(d));
      }
      grad[idx] = v;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------------------------ (c)
__device__ void fwd_c(const float* __restrict__ x, const long long* __restrict__ label, const float* mask, int form, int B, int S2, Scratch& s,
                      float* out) {
  float s1 = 0.f, s0 = 0.f;
  int n1 = 0, n0 = 0;
  for (int i = threadIdx.x; i < B * S2; i += T) {
    const int b = i / S2, c = i - b * S2;
    if (!sample_on(mask, b)) continue;
    const long long L = label[i];
    if (L != 0 && L != 1) continue;
    float v0, v1;
    load2(x, form, b, c, S2, v0, v1);
    if (form == 0) {
      const Soft2 lp = log_softmax2(v0, v1);
      v0 = lp.p0, v1 = lp.p1;
    }
    if (L == 1) {
      s1 = rn_sub(s1, v1);
      ++n1;
    } else {
      s0 = rn_sub(s0, v0);
      ++n0;
    }
  }
  n1 = block_sum<NW>(n1, s.i);
  n0 = block_sum<NW>(n0, s.i);
  s1 = block_sum<NW>(s1, s.f);
  s0 = block_sum<NW>(s0, s.f);
  const float pos = n1 <= 1 ? 0.f : rn_div(s1, (float)n1), neg = n0 <= 1 ? 0.f : rn_div(s0, (float)n0);
  if (threadIdx.x == 0) *out = rn_add(rn_mul(pos, 0.5f), rn_mul(neg, 0.5f));
}

__device__ void bwd_c(const float* __restrict__ x, const long long* __restrict__ label, const float* mask, int form, int B, int S2, Scratch& s,
                      float g, float* __restrict__ grad) {
  int n1 = 0, n0 = 0;
  for (int i = threadIdx.x; i < B * S2; i += T)
    if (sample_on(mask, i / S2)) {
      n1 += label[i] == 1;
      n0 += label[i] == 0;
    }
  n1 = block_sum<NW>(n1, s.i);
  n0 = block_sum<NW>(n0, s.i);
  const float u1 = n1 <= 1 ? 0.f : -rn_div(rn_mul(0.5f, g), (float)n1), u0 = n0 <= 1 ? 0.f : -rn_div(rn_mul(0.5f, g), (float)n0);
  for (int i = threadIdx.x; i < B * S2; i += T) {
    const int b = i / S2, c = i - b * S2;
    float a0 = 0.f, a1 = 0.f;                        // d loss / d logp of the cell
    if (sample_on(mask, b)) {
      const long long L = label[i];
      if (L == 1) a1 = u1; else if (L == 0) a0 = u0;
    }
    if (form == 0) {
      float g0 = 0.f, g1 = 0.f;
      if (a0 != 0.f || a1 != 0.f) {
        float v0, v1;
        load2(x, 0, b, c, S2, v0, v1);
        const Soft2 sm = softmax2(v0, v1);
        const float tot = rn_add(a0, a1);             // log_softmax backward: a_j - softmax_j (a_0 + a_1)
        g0 = rn_sub(a0, rn_mul(sm.p0, tot));
        g1 = rn_sub(a1, rn_mul(sm.p1, tot));
      }
      grad[(b * 2 + 0) * S2 + c] = g0;
      grad[(b * 2 + 1) * S2 + c] = g1;
    } else {
      grad[(b * S2 + c) * 2 + 0] = a0;
      grad[(b * S2 + c) * 2 + 1] = a1;
    }
  }
}

struct Args {
  const float *cls, *label_cls, *loc, *label_loc, *cls_lp;
  const long long* label_cls_lp;
  const float *loc_lp, *label_loc_lp, *rows, *rows_tgt, *mask;
  int B, S2, S2lp, n_rows, C, topk, form;
};

__global__ __launch_bounds__(T) void fwd_kernel(Args a, float* __restrict__ losses) {
  extern __shared__ unsigned lb[];
  __shared__ Scratch s;
  switch (blockIdx.x) {
    case 0:
      if (a.cls) fwd_a(a.cls, a.label_cls, a.mask, a.form, a.B, a.S2, a.topk, lb, s, losses + 0);
      break;
    case 1:
      if (a.loc) fwd_smooth(a.loc, a.label_loc, 1, a.label_cls, nullptr, a.mask, a.B, 2, a.S2, true, s, losses + 1);
      break;
    case 2:
      if (a.cls_lp) fwd_c(a.cls_lp, a.label_cls_lp, a.mask, a.form, a.B, a.S2lp, s, losses + 2);
      break;
    case 3:
      if (a.loc_lp) fwd_smooth(a.loc_lp, a.label_loc_lp, 2, nullptr, a.label_cls_lp, a.mask, a.B, 4, a.S2lp, false, s, losses + 3);
      break;
    default:
      if (a.rows) fwd_smooth(a.rows, a.rows_tgt, 0, nullptr, nullptr, nullptr, a.n_rows, a.C, 1, false, s, losses + 4);
  }
}

struct Grads {
  float *cls, *loc, *cls_lp, *loc_lp, *rows;
};

__global__ __launch_bounds__(T) void bwd_kernel(Args a, const float* __restrict__ gl, Grads g) {
  extern __shared__ unsigned lb[];
  __shared__ Scratch s;
  switch (blockIdx.x) {
    case 0:
      if (g.cls) bwd_a(a.cls, a.label_cls, a.mask, a.form, a.B, a.S2, a.topk, lb, s, gl[0], g.cls);
      break;
    case 1:
      if (g.loc) bwd_smooth(a.loc, a.label_loc, 1, a.label_cls, nullptr, a.mask, a.B, 2, a.S2, true, s, gl[1], g.loc);
      break;
    case 2:
      if (g.cls_lp) bwd_c(a.cls_lp, a.label_cls_lp, a.mask, a.form, a.B, a.S2lp, s, gl[2], g.cls_lp);
      break;
    case 3:
      if (g.loc_lp) bwd_smooth(a.loc_lp, a.label_loc_lp, 2, nullptr, a.label_cls_lp, a.mask, a.B, 4, a.S2lp, false, s, gl[3], g.loc_lp);
      break;
    default:
      if (g.rows) bwd_smooth(a.rows, a.rows_tgt, 0, nullptr, nullptr, nullptr, a.n_rows, a.C, 1, false, s, gl[4], g.rows);
  }
}

struct Range {
  const void* p;
  long long bytes;
};

// NULL, shape and limit rules shared by the two entries; on HDN_OK fills `a` and the byte ranges of every input that is present
static int prepare(Args& a, Range* in, int& n_in, bool want[5]) {
  const bool has_a = a.cls, has_b = a.loc, has_c = a.cls_lp, has_d = a.loc_lp, has_e = a.rows || a.rows_tgt;
  if (has_a && !a.label_cls) return HDN_E_NULL;
  if (has_b && (!a.label_loc || !a.label_cls)) return HDN_E_NULL;
  if (has_c && !a.label_cls_lp) return HDN_E_NULL;
  if (has_d && (!a.label_loc_lp || !a.label_cls_lp)) return HDN_E_NULL;
  if (has_e && (!a.rows || !a.rows_tgt)) return HDN_E_NULL;
  if (!has_a && !has_b && !has_c && !has_d && !has_e) return HDN_E_NULL;
  const bool maps = has_a || has_b, maps_lp = has_c || has_d;
  const int S = a.S2, Slp = a.S2lp;      // the sides on entry
  if ((a.form != 0 && a.form != 1) || (a.form == 1 && a.mask)) return HDN_E_SHAPE;
  if ((maps || maps_lp) && a.B <= 0) return HDN_E_SHAPE;
  if (maps && S <= 0) return HDN_E_SHAPE;
  if (maps_lp && Slp <= 0) return HDN_E_SHAPE;
  if (has_a && a.topk <= 0) return HDN_E_SHAPE;
  if (has_e && (a.n_rows <= 0 || a.C <= 0)) return HDN_E_SHAPE;
  if (maps && (long long)a.B * S * S > MAX_CELLS) return HDN_E_LIMIT;
  if (maps_lp && (long long)a.B * Slp * Slp > MAX_CELLS) return HDN_E_LIMIT;
  if (has_e && (long long)a.n_rows * a.C > MAX_ROW_ELEMS) return HDN_E_LIMIT;
  a.S2 = maps ? S * S : 1;
  a.S2lp = maps_lp ? Slp * Slp : 1;
  const long long cells = (long long)a.B * a.S2, cells_lp = (long long)a.B * a.S2lp, re = (long long)a.n_rows * a.C;
  n_in = 0;
  auto add = [&](const void* p, long long bytes) {
    if (p) in[n_in++] = {p, bytes};
  };
  add(a.cls, cells * 8), add(a.label_cls, cells * 4), add(a.loc, cells * 8), add(a.label_loc, cells * 8), add(a.cls_lp, cells_lp * 8);
  add(a.label_cls_lp, cells_lp * 8), add(a.loc_lp, cells_lp * 16), add(a.label_loc_lp, cells_lp * 16), add(a.rows, re * 4), add(a.rows_tgt, re * 4);
  add(a.mask, (long long)a.B * 4);
  want[0] = has_a, want[1] = has_b, want[2] = has_c, want[3] = has_d, want[4] = has_e;
  return HDN_OK;
}

static int lds_bytes(const Args& a, bool with_a) { return with_a ? a.B * a.S2 * 4 : 0; }

}  // namespace sup
}  // namespace hdn

extern "C" {

int hdn_sup_losses_f32(const float* cls, const float* label_cls, const float* loc, const float* label_loc_c, const float* cls_lp,
                       const long long* label_cls_lp, const float* loc_lp, const float* label_loc_lp, const float* rows, const float* rows_target,
                       const float* if_unsup_or_null, float* losses, int B, int S, int S_lp, int n_rows, int C, int topk_per_sample, int form,
                       void* stream) {
  using namespace hdn;
  sup::Args a{cls, label_cls, loc, label_loc_c, cls_lp, label_cls_lp, loc_lp, label_loc_lp, rows, rows_target, if_unsup_or_null,
              B,   S,         S_lp, n_rows,     C,      topk_per_sample, form};
  if (!losses) return HDN_E_NULL;
  sup::Range in[11];
  int n_in = 0;
  bool want[5];
  if (const int rc = sup::prepare(a, in, n_in, want)) return rc;
  for (int i = 0; i < n_in; ++i)
    if (bytes_overlap(losses, 20, in[i].p, in[i].bytes)) return HDN_E_ALIAS;
  static PerDeviceOnce once;
  if (const int rc = lds_opt_in(once, sup::MAX_CELLS * 4, sup::fwd_kernel)) return rc;
  hipLaunchKernelGGL(sup::fwd_kernel, dim3(5), dim3(sup::T), sup::lds_bytes(a, want[0]), static_cast<hipStream_t>(stream), a, losses);
  return launch_status();
}

int hdn_sup_losses_bwd_f32(const float* cls, const float* label_cls, const float* loc, const float* label_loc_c, const float* cls_lp,
                           const long long* label_cls_lp, const float* loc_lp, const float* label_loc_lp, const float* rows,
                           const float* rows_target, const float* if_unsup_or_null, const float* grad_losses, float* grad_cls_or_null,
                           float* grad_loc_or_null, float* grad_cls_lp_or_null, float* grad_loc_lp_or_null, float* grad_rows_or_null, int B, int S,
                           int S_lp, int n_rows, int C, int topk_per_sample, int form, void* stream) {
  using namespace hdn;
  sup::Args a{cls, label_cls, loc, label_loc_c, cls_lp, label_cls_lp, loc_lp, label_loc_lp, rows, rows_target, if_unsup_or_null,
              B,   S,         S_lp, n_rows,     C,      topk_per_sample, form};
  if (!grad_losses) return HDN_E_NULL;
  float* const outs[5] = {grad_cls_or_null, grad_loc_or_null, grad_cls_lp_or_null, grad_loc_lp_or_null, grad_rows_or_null};
  sup::Range in[12];
  int n_in = 0;
  bool want[5];
  const bool present[5] = {cls != nullptr, loc != nullptr, cls_lp != nullptr, loc_lp != nullptr, rows != nullptr};
  for (int i = 0; i < 5; ++i)
    if (outs[i] && !present[i]) return HDN_E_NULL;           // a gradient of a loss whose inputs are not given
  if (const int rc = sup::prepare(a, in, n_in, want)) return rc;
  if (!outs[0] && !outs[1] && !outs[2] && !outs[3] && !outs[4]) return HDN_E_SHAPE;
  in[n_in++] = {grad_losses, 20};
  const long long cells = (long long)a.B * a.S2, cells_lp = (long long)a.B * a.S2lp;
  const long long out_bytes[5] = {cells * 8, cells * 8, cells_lp * 8, cells_lp * 16, (long long)a.n_rows * a.C * 4};
  for (int i = 0; i < 5; ++i) {
    if (!outs[i]) continue;
    for (int j = 0; j < n_in; ++j)
      if (bytes_overlap(outs[i], out_bytes[i], in[j].p, in[j].bytes)) return HDN_E_ALIAS;
    for (int j = 0; j < i; ++j)
      if (outs[j] && bytes_overlap(outs[i], out_bytes[i], outs[j], out_bytes[j])) return HDN_E_ALIAS;
  }
  static PerDeviceOnce once;
  if (const int rc = lds_opt_in(once, sup::MAX_CELLS * 4, sup::bwd_kernel)) return rc;
  const sup::Grads g{outs[0], outs[1], outs[2], outs[3], outs[4]};
  hipLaunchKernelGGL(sup::bwd_kernel, dim3(5), dim3(sup::T), sup::lds_bytes(a, outs[0] != nullptr), static_cast<hipStream_t>(stream), a, grad_losses, g);
  return launch_status();
}

}  // extern "C"
