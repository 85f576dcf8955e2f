// The optimizer stretch of a training iteration (tools/train.py:271-281 of the reference: is_valid_number(loss), clip_grad_norm_, Adam(amsgrad=True)
// .step()) for gfx950, with nothing read by or uploaded from the host:
//
//   hdn_grad_sqnorm_f32     one float64 partial sum of squares per CHUNK elements of every gradient, at a place fixed by the sizes alone
//   hdn_opt_gate_f32        ONE workgroup: the partials added in a fixed order -> grad_norm, the loss / norm gate -> status, clip_coef, and for a
//                           step that is taken the counters and the two bias-correction factors of every tensor that has a gradient
//   hdn_amsgrad_apply_f32   the element-wise update; returns after reading status when the step is skipped
//
// The formulas are in include/hdn_hip.h.  Parameter and gradient pointers reach the kernels BY VALUE, in a table of at most TENSORS entries that is
// the kernel's argument (gradients are allocated inside a graph capture, so no table built beforehand on the device can know them); more tensors
// take more launches.  A launch's work items are chunks of CHUNK elements; chunk0[] is the running count of chunks, a workgroup finds the tensor of
// its chunk by bisection (uniform: scalar loads from the argument segment) and walks the chunks grid-stride, the grid capped at MAX_GRID workgroups.
// The moments are three flat buffers; tensor i's slot starts at the sum of the earlier sizes, each rounded up to 4 floats (16 bytes).
//
// A chunk takes the 16-byte path when its parameter and gradient pointers are 16-byte aligned (the slot always is), with the last numel % 4
// elements on the scalar path; a misaligned view takes the scalar path throughout.  Index arithmetic is 64-bit.  No atomics: every partial and
// every element has one writer, sums have a fixed order, so the same inputs give the same bits, launched or replayed.
// Bounds: chunk c of tensor t covers elements [c CHUNK, min(numel, (c + 1) CHUNK)) of p, g and slot[t] + the same of the moments; the entry point
// checks slot[t] + numel[t] <= state_floats and the partial count before any launch.
#include "hdn_common.h"
#include "reduce.h"

#include <math.h>

#pragma clang fp contract(off)

namespace hdn {
namespace opt {

constexpr int TENSORS = 96;
constexpr int CHUNK = 4096;
constexpr int MAX_GRID = 2048;
constexpr int MASK_WORDS = 896;                   // gate: one bit per tensor, by value
constexpr long long MAX_NUMEL = 1ll << 40;

struct NormTable {
  const float* g[TENSORS];
  long long numel[TENSORS];
  int chunk0[TENSORS + 1];
  int n;
};
struct ApplyTable {
  float* p[TENSORS];
  float* g[TENSORS];
  long long numel[TENSORS];
  long long slot[TENSORS];
  int chunk0[TENSORS + 1];
  int n;
  int first;                                      // the index of entry 0 among the optimizer's tensors (coef[])
};
struct GradMask {
  unsigned int w[MASK_WORDS];
};
static_assert(sizeof(NormTable) + 64 <= 4096 && sizeof(ApplyTable) + 128 <= 4096 && sizeof(GradMask) + 256 <= 4096, "a launch's arguments stay within 4 KB");

// the entry t with chunk0[t] <= chunk < chunk0[t + 1] (entries without chunks are skipped by the strict upper bound)
__device__ __forceinline__ int find_tensor(const int* chunk0, int n, int chunk) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (chunk0[mid] <= chunk) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(HDN_BLOCK) void sqnorm_kernel(const NormTable tb, double* __restrict__ partials) {
  __shared__ double red[BLOCK_WAVES];
  const int tid = threadIdx.x;
  const int total = tb.chunk0[tb.n];
  for (int chunk = blockIdx.x; chunk < total; chunk += gridDim.x) {
    const int t = find_tensor(tb.chunk0, tb.n, chunk);
    const float* g = tb.g[t];
    double acc = 0.0;
    if (g) {
      const long long base = (long long)(chunk - tb.chunk0[t]) * CHUNK;
      const long long left = tb.numel[t] - base;
      const int count = left < CHUNK ? (int)left : CHUNK;
      g += base;
      if (aligned16(g)) {
        const int n4 = count >> 2;
        const float4* g4 = reinterpret_cast<const float4*>(g);
        for (int i = tid; i < n4; i += HDN_BLOCK) {
          const float4 q = g4[i];
          acc += (double)q.x * (double)q.x;
          acc += (double)q.y * (double)q.y;
          acc += (double)q.z * (double)q.z;
          acc += (double)q.w * (double)q.w;
        }
        const int i = (n4 << 2) + tid;
        if (i < count) acc += (double)g[i] * (double)g[i];
      } else {
        for (int i = tid; i < count; i += HDN_BLOCK) acc += (double)g[i] * (double)g[i];
      }
    }
    acc = block_sum<BLOCK_WAVES>(acc, red);  // its leading barrier: red is written again in the next round
    if (tid == 0) partials[chunk] = acc;
  }
}

// ctrl: [0] status (int32), [1] grad_norm, [2] clip_coef, [3] unused.  coef: step_size[n] then inv_sqrt_bc2[n].
__global__ __launch_bounds__(HDN_BLOCK) void gate_kernel(const double* __restrict__ partials, long long n_partials, const float* __restrict__ loss,
                                                         float loss_limit, int clip, double max_norm, const double* __restrict__ lr,
                                                         const int* __restrict__ group, const GradMask mask, int n, double beta1, double beta2,
                                                         float* __restrict__ ctrl, float* __restrict__ steps, float* __restrict__ coef) {
  __shared__ double red[HDN_BLOCK];
  __shared__ int status_s;
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (long long i = tid; i < n_partials; i += HDN_BLOCK) acc += partials[i];
  red[tid] = acc;  // not reduce.h's order: a 256-slot LDS tree over doubles (strides 128 .. 1), kept because grad_norm's bits are pinned by it
  __syncthreads();
  for (int s = HDN_BLOCK / 2; s >= 1; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) {
    const double norm = sqrt(red[0]);
    int status = 0;
    if (loss) {
      const float x = *loss;
      if (isnan(x) || isinf(x) || x > loss_limit) status = 1;
    }
    if (status == 0 && !isfinite(norm)) status = 2;
    double c = 1.0;
    if (clip) {
      c = max_norm / (norm + 1e-6);
      c = c < 1.0 ? c : 1.0;                      // NaN (status 2) -> 1; never used then
    }
    reinterpret_cast<int*>(ctrl)[0] = status;
    ctrl[1] = (float)norm;
    ctrl[2] = (float)c;
    status_s = status;
  }
  __syncthreads();
  if (status_s != 0) return;
  for (int i = tid; i < n; i += HDN_BLOCK) {
    if (!((mask.w[i >> 5] >> (i & 31)) & 1u)) continue;
    const float t = steps[i] + 1.f;
    steps[i] = t;
    coef[i] = (float)(lr[group[i]] / (1.0 - pow(beta1, (double)t)));
    coef[n + i] = (float)(1.0 / sqrt(1.0 - pow(beta2, (double)t)));
  }
}

struct Hyper {
  float c, b1, omb1, b2, omb2, eps, wd, step_size, inv_sqrt_bc2;
};

// one element: g = c g + wd p; m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g g; vmax = max(vmax, v); p -= step_size m / (sqrt(vmax) inv + eps),
// every operation rounded on its own (contraction is off in this file), sqrt and / correctly rounded
__device__ __forceinline__ void update(const Hyper& h, float& p, float& g, float& m, float& v, float& vmax) {
  g = h.c * g;
  const float ge = g + h.wd * p;
  m = h.b1 * m + h.omb1 * ge;
  v = h.b2 * v + (h.omb2 * ge) * ge;
  vmax = fmaxf(vmax, v);
  p = p - (h.step_size * m) / (__fsqrt_rn(vmax) * h.inv_sqrt_bc2 + h.eps);
}

__global__ __launch_bounds__(HDN_BLOCK) void apply_kernel(const ApplyTable tb, float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq,
                                                          float* __restrict__ max_exp_avg_sq, const float* __restrict__ ctrl,
                                                          const float* __restrict__ coef, int n_all, float b1, float omb1, float b2, float omb2,
                                                          float eps, float wd, int write_grads) {
  if (reinterpret_cast<const int*>(ctrl)[0] != 0) return;  // a skipped step: nothing is written
  const int tid = threadIdx.x;
  Hyper h;
  h.c = ctrl[2], h.b1 = b1, h.omb1 = omb1, h.b2 = b2, h.omb2 = omb2, h.eps = eps, h.wd = wd;
  const int total = tb.chunk0[tb.n];
  for (int chunk = blockIdx.x; chunk < total; chunk += gridDim.x) {
    const int t = find_tensor(tb.chunk0, tb.n, chunk);
    const long long base = (long long)(chunk - tb.chunk0[t]) * CHUNK;
    const long long left = tb.numel[t] - base;
    const int count = left < CHUNK ? (int)left : CHUNK;
    float* p = tb.p[t] + base;
    float* g = tb.g[t] + base;
    float* m = exp_avg + tb.slot[t] + base;
    float* v = exp_avg_sq + tb.slot[t] + base;
    float* x = max_exp_avg_sq + tb.slot[t] + base;
    h.step_size = coef[tb.first + t];
    h.inv_sqrt_bc2 = coef[n_all + tb.first + t];
    const bool vec = aligned16(p) && aligned16(g);
    const int n4 = vec ? count >> 2 : 0;
    for (int i = tid; i < n4; i += HDN_BLOCK) {
      float4 p4 = reinterpret_cast<float4*>(p)[i], g4 = reinterpret_cast<float4*>(g)[i];
      float4 m4 = reinterpret_cast<float4*>(m)[i], v4 = reinterpret_cast<float4*>(v)[i], x4 = reinterpret_cast<float4*>(x)[i];
      update(h, p4.x, g4.x, m4.x, v4.x, x4.x);
      update(h, p4.y, g4.y, m4.y, v4.y, x4.y);
      update(h, p4.z, g4.z, m4.z, v4.z, x4.z);
      update(h, p4.w, g4.w, m4.w, v4.w, x4.w);
      reinterpret_cast<float4*>(p)[i] = p4;
      reinterpret_cast<float4*>(m)[i] = m4;
      reinterpret_cast<float4*>(v)[i] = v4;
      reinterpret_cast<float4*>(x)[i] = x4;
      if (write_grads) reinterpret_cast<float4*>(g)[i] = g4;
    }
    for (int i = (n4 << 2) + tid; i < count; i += HDN_BLOCK) {  // the tail, or a misaligned view as a whole
      float pv = p[i], gv = g[i], mv = m[i], vv = v[i], xv = x[i];
      update(h, pv, gv, mv, vv, xv);
      p[i] = pv, m[i] = mv, v[i] = vv, x[i] = xv;
      if (write_grads) g[i] = gv;
    }
  }
}

inline long long chunks_of(long long numel) { return (numel + CHUNK - 1) / CHUNK; }
inline int grid_of(int chunks) { return chunks < MAX_GRID ? chunks : MAX_GRID; }

// numel[0..n): each in [0, MAX_NUMEL]
inline int check_numel(const long long* numel, int n) {
  for (int i = 0; i < n; ++i) {
    if (numel[i] < 0) return HDN_E_SHAPE;
    if (numel[i] > MAX_NUMEL) return HDN_E_LIMIT;
  }
  return HDN_OK;
}

}  // namespace opt
}  // namespace hdn

extern "C" {

int hdn_opt_tensors_per_launch(void) { return hdn::opt::TENSORS; }
int hdn_opt_chunk(void) { return hdn::opt::CHUNK; }

long long hdn_grad_sqnorm_partials(const long long* numel, int n) {
  using namespace hdn;
  if (n < 0 || (n > 0 && !numel)) return n < 0 ? HDN_E_SHAPE : HDN_E_NULL;
  if (const int rc = opt::check_numel(numel, n)) return rc;
  long long total = 0;
  for (int i = 0; i < n; ++i) total += opt::chunks_of(numel[i]);
  return total;
}

long long hdn_opt_state_floats(const long long* numel, int n) {
  using namespace hdn;
  if (n < 0 || (n > 0 && !numel)) return n < 0 ? HDN_E_SHAPE : HDN_E_NULL;
  if (const int rc = opt::check_numel(numel, n)) return rc;
  long long total = 0;
  for (int i = 0; i < n; ++i) total += (numel[i] + 3) / 4 * 4;
  return total;
}

int hdn_grad_sqnorm_f32(const float* const* grads, const long long* numel, int n, double* partials, long long n_partials, void* stream) {
  using namespace hdn;
  if (n < 0) return HDN_E_SHAPE;
  if (n == 0) return HDN_OK;
  if (!grads || !numel || !partials) return HDN_E_NULL;
  const long long need = hdn_grad_sqnorm_partials(numel, n);
  if (need < 0) return (int)need;
  if (n_partials < need || (reinterpret_cast<uintptr_t>(partials) & 7u)) return HDN_E_LIMIT;
  for (int i = 0; i < n; ++i)
    if (reinterpret_cast<uintptr_t>(grads[i]) & 3u) return HDN_E_LIMIT;
  long long done = 0;
  for (int first = 0; first < n;) {
    opt::NormTable tb;
    int k = 0;
    long long chunks = 0;
    for (; first + k < n && k < opt::TENSORS; ++k) {
      const long long c = opt::chunks_of(numel[first + k]);
      if (chunks + c > (1ll << 30)) break;
      tb.g[k] = grads[first + k];
      tb.numel[k] = numel[first + k];
      tb.chunk0[k] = (int)chunks;
      chunks += c;
    }
    if (k == 0) return HDN_E_LIMIT;
    tb.chunk0[k] = (int)chunks;
    tb.n = k;
    if (chunks > 0) {
      hipLaunchKernelGGL(opt::sqnorm_kernel, dim3(opt::grid_of((int)chunks)), dim3(HDN_BLOCK), 0, static_cast<hipStream_t>(stream), tb,
                         partials + done);
      if (const int rc = launch_status()) return rc;
    }
    done += chunks;
    first += k;
  }
  return HDN_OK;
}

int hdn_opt_gate_f32(const double* partials, long long n_partials, const float* loss_or_null, float loss_limit, int clip, double max_norm,
                     const double* lr, const int* group, const float* const* grads, int n, double beta1, double beta2, float* ctrl, float* steps,
                     float* coef, void* stream) {
  using namespace hdn;
  if (!ctrl || (n_partials > 0 && !partials)) return HDN_E_NULL;
  if (n > 0 && (!lr || !group || !grads || !steps || !coef)) return HDN_E_NULL;
  if (n < 0 || n_partials < 0 || (clip && !(max_norm > 0.0)) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return HDN_E_SHAPE;
  if (n > opt::MASK_WORDS * 32) return HDN_E_LIMIT;
  opt::GradMask mask;
  for (int w = 0; w < (n + 31) / 32; ++w) mask.w[w] = 0u;
  for (int i = 0; i < n; ++i)
    if (grads[i]) mask.w[i >> 5] |= 1u << (i & 31);
  hipLaunchKernelGGL(opt::gate_kernel, dim3(1), dim3(HDN_BLOCK), 0, static_cast<hipStream_t>(stream), partials, n_partials, loss_or_null,
                     loss_limit, clip, max_norm, lr, group, mask, n, beta1, beta2, ctrl, steps, coef);
  return launch_status();
}

int hdn_amsgrad_apply_f32(float* const* params, float* const* grads, const long long* numel, int n, float* exp_avg, float* exp_avg_sq,
                          float* max_exp_avg_sq, long long state_floats, const float* ctrl, const float* coef, double beta1, double beta2,
                          double eps, double weight_decay, int write_grads, void* stream) {
  using namespace hdn;
  if (n < 0) return HDN_E_SHAPE;
  if (n == 0) return HDN_OK;
  if (!params || !grads || !numel || !exp_avg || !exp_avg_sq || !max_exp_avg_sq || !ctrl || !coef) return HDN_E_NULL;
  const long long need = hdn_opt_state_floats(numel, n);
  if (need < 0) return (int)need;
  if (state_floats < need || !aligned16(exp_avg) || !aligned16(exp_avg_sq) || !aligned16(max_exp_avg_sq)) return HDN_E_LIMIT;
  for (int i = 0; i < n; ++i) {
    if (!params[i]) return HDN_E_NULL;
    if ((reinterpret_cast<uintptr_t>(params[i]) & 3u) || (reinterpret_cast<uintptr_t>(grads[i]) & 3u)) return HDN_E_LIMIT;
    if (grads[i] && bytes_overlap(params[i], numel[i] * 4, grads[i], numel[i] * 4)) return HDN_E_ALIAS;
  }
  long long slot = 0;
  for (int first = 0; first < n;) {
    opt::ApplyTable tb;
    int k = 0;
    long long chunks = 0;
    for (; first + k < n && k < opt::TENSORS; ++k) {
      const long long c = grads[first + k] ? opt::chunks_of(numel[first + k]) : 0;  // no gradient: no work, the slot stays where it is
      if (chunks + c > (1ll << 30)) break;
      tb.p[k] = params[first + k];
      tb.g[k] = grads[first + k];
      tb.numel[k] = numel[first + k];
      tb.slot[k] = slot;
      tb.chunk0[k] = (int)chunks;
      chunks += c;
      slot += (numel[first + k] + 3) / 4 * 4;
    }
    if (k == 0) return HDN_E_LIMIT;
    tb.chunk0[k] = (int)chunks;
    tb.n = k;
    tb.first = first;
    if (chunks > 0) {
      hipLaunchKernelGGL(opt::apply_kernel, dim3(opt::grid_of((int)chunks)), dim3(HDN_BLOCK), 0, static_cast<hipStream_t>(stream), tb, exp_avg,
                         exp_avg_sq, max_exp_avg_sq, ctrl, coef, n, (float)beta1, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2),
                         (float)eps, (float)weight_decay, write_grads);
      if (const int rc = launch_status()) return rc;
    }
    first += k;
  }
  return HDN_OK;
}

}  // extern "C"
