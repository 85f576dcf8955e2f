// PreShareFeature with batch statistics, forward and backward, for gfx950 (training): hdn_share_feature_train_fwd_f32 and hdn_share_feature_bwd_f32.
// The formulas and the buffer layouts are in include/hdn_hip.h.  share_feature.hip (the fused eval kernel) is untouched.
//
// Batch statistics put a global reduction between the layers, so the chain is layered: per layer one "convolution + partial sums" launch over the
// previous layer's PRE-normalisation planes (relu(c alpha + beta) is applied on load from the 13-entry table in the workspace; the activations are
// never stored) and a one-workgroup finish that turns the partials into mean / invstd / unbiased variance and the next table entries.  The backward
// walks the layers down: reduce (S1, S2), apply (dc), then the convolution's two adjoints, both gathers.
//
// One launch form: a workgroup of HDN_BLOCK threads owns PXB = 1024 consecutive pixels of one image (row-major H W), thread t the pixels
// t, t + 256, t + 512, t + 768 of them, so a wave's loads are contiguous.  The 3x3 taps are read from global memory (L1 / L2 hits: a 127 x 127 plane
// is 64 KB and the whole step is launch- and bandwidth-bound); padding is zero in activation space, so a tap outside the plane contributes 0, not
// relu(beta).
//
// Every sum over pixels is deterministic and uses no atomics: a thread adds its pixels in ascending order, the workgroup adds its threads in the fixed
// order of reduce.h and writes one partial into the workspace; the finish launch adds the partials in a fixed order (thread t takes partials
// t, t + T, ..., then the same reduction).  The statistics and S1 / S2 are carried in float64 from the
// first add on (fp64 adds are not the limit here); the weight gradients add fp32 products in fp32 inside a workgroup (1024 terms, a tree) and in
// float64 across workgroups.  grad_img is a gather like every other plane, so it is bit-reproducible too.
#include "hdn_common.h"
#include "reduce.h"

namespace hdn {
namespace sft {

constexpr int WAVES = BLOCK_WAVES;
constexpr int PX = 4;                 // pixels per thread
constexpr int PXB = HDN_BLOCK * PX;    // pixels per workgroup
constexpr int NCH = 13;                // 4 + 8 + 1 BatchNorm channels, layers concatenated
constexpr int NPAR = 36 + 288 + 72 + 13 + 13;
// workspace, in floats: [0,13) alpha, [13,26) beta, [32,45) S1, [48,61) S2, then the partials, then two groups of 8 planes
constexpr int WS_ALPHA = 0, WS_BETA = 13, WS_S1 = 32, WS_S2 = 48, WS_HEAD = 64;
constexpr int PART_FLOATS = 288;       // per workgroup: the largest user is layer 2's weight gradient (8 x 4 x 9 floats); 16 doubles fit as well

// alpha = gamma invstd, beta = bias - mean alpha (one rounding), from the fp32 statistics: forward and backward build the same table
__device__ __forceinline__ void make_ab(float gamma, float bias, float mean, float invstd, float* alpha, float* beta) {
  const float a = rn_mul(gamma, invstd);
  *alpha = a;
  *beta = __builtin_fmaf(-mean, a, bias);
}

// p[0], p[stride], ... p[(n - 1) stride] added in a fixed order by the whole workgroup; every thread gets the sum.  lds: WAVES doubles.
__device__ __forceinline__ double block_total(const double* __restrict__ p, int n, int stride, double* lds) {
  double s = 0.0;
  for (int k = threadIdx.x; k < n; k += HDN_BLOCK) s += p[size_t(k) * stride];
  return block_sum<WAVES>(s, lds);
}

// the activation a = relu(c alpha + beta) of one input channel at (y, x), 0 outside the plane; FIRST: the plane is the image itself
template <bool FIRST>
__device__ __forceinline__ float act_at(const float* __restrict__ plane, int y, int x, int H, int W, float alpha, float beta) {
  if ((unsigned)y >= (unsigned)H || (unsigned)x >= (unsigned)W) return 0.f;
  const float c = plane[y * W + x];
  return FIRST ? c : fmaxf(__builtin_fmaf(c, alpha, beta), 0.f);
}

// ---------------------------------------------------------------------------------------------------------------- forward
// c_out[b][co] = conv3x3(a_in)[co], and (part != NULL) the workgroup's sums of c and c^2 per output channel: part[blk][2 co], part[blk][2 co + 1]
template <int CI, int CO, bool FIRST>
__global__ __launch_bounds__(HDN_BLOCK) void conv_stats_kernel(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ tab,
                                                               float* __restrict__ out, double* __restrict__ part, int H, int W, int nbx) {
  __shared__ double red[WAVES * 2 * CO];
  const int b = blockIdx.x / nbx, bx = blockIdx.x - b * nbx;
  const int HW = H * W;
  const float* ib = in + size_t(b) * CI * HW;
  float* ob = out + size_t(b) * CO * HW;
  float al[CI], be[CI];
#pragma unroll
  for (int ci = 0; ci < CI; ++ci) {
    al[ci] = FIRST ? 1.f : tab[WS_ALPHA + ci];
    be[ci] = FIRST ? 0.f : tab[WS_BETA + ci];
  }
  double sums[2 * CO];
#pragma unroll
  for (int q = 0; q < 2 * CO; ++q) sums[q] = 0.0;
#pragma unroll 1
  for (int i = 0; i < PX; ++i) {
    const int pix = bx * PXB + i * HDN_BLOCK + threadIdx.x;
    if (pix >= HW) continue;
    const int y = pix / W, x = pix - y * W;
    float acc[CO];
#pragma unroll
    for (int co = 0; co < CO; ++co) acc[co] = 0.f;
#pragma unroll
    for (int ci = 0; ci < CI; ++ci) {
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const float a = act_at<FIRST>(ib + size_t(ci) * HW, y + k / 3 - 1, x + k % 3 - 1, H, W, al[ci], be[ci]);
#pragma unroll
        for (int co = 0; co < CO; ++co) acc[co] = __builtin_fmaf(w[(co * CI + ci) * 9 + k], a, acc[co]);
      }
    }
#pragma unroll
    for (int co = 0; co < CO; ++co) {
      ob[size_t(co) * HW + pix] = acc[co];
      const double d = (double)acc[co];
      sums[2 * co] += d;
      sums[2 * co + 1] += d * d;
    }
  }
  if (part) block_sum_store<2 * CO, WAVES>(sums, red, part + size_t(blockIdx.x) * 2 * CO);  // kernel-uniform branch
}

// one workgroup: the partials of CO channels -> mean, invstd, unbiased variance (stats[ch0 ..], three rows of NCH) and the table entries
__global__ __launch_bounds__(HDN_BLOCK) void stats_finish_kernel(const double* __restrict__ part, int nblk, int CO, int ch0, double n, double eps,
                                                                 const float* __restrict__ gamma, const float* __restrict__ bias,
                                                                 float* __restrict__ stats, float* __restrict__ tab) {
  __shared__ double red[WAVES];
  for (int co = 0; co < CO; ++co) {
    const double s = block_total(part + 2 * co, nblk, 2 * CO, red);
    const double q = block_total(part + 2 * co + 1, nblk, 2 * CO, red);
    if (threadIdx.x == 0) {
      const double mean = s / n;
      const double var = fmax(q / n - mean * mean, 0.0);
      const float mean_f = (float)mean, invstd_f = (float)(1.0 / sqrt(var + eps));
      const int ch = ch0 + co;
      stats[ch] = mean_f;
      stats[NCH + ch] = invstd_f;
      stats[2 * NCH + ch] = (float)(var * (n / (n - 1.0)));
      make_ab(gamma[ch], bias[ch], mean_f, invstd_f, tab + WS_ALPHA + ch, tab + WS_BETA + ch);
    }
  }
}

// the whole table at once.  mean_var != NULL (frozen statistics, forward): stats = (mean, 1 / sqrt(var + eps), var) first.  Else stats is read (backward).
__global__ void table_kernel(const float* __restrict__ mean_var, float eps1, float eps2, float eps3, const float* __restrict__ gamma,
                             const float* __restrict__ bias, float* __restrict__ stats_w, const float* __restrict__ stats_r, float* __restrict__ tab) {
  const int ch = threadIdx.x;
  if (ch >= NCH) return;
  float mean, invstd;
  if (mean_var) {
    const double eps = (double)(ch < 4 ? eps1 : (ch < 12 ? eps2 : eps3));
    mean = mean_var[ch];
    invstd = (float)(1.0 / sqrt((double)mean_var[NCH + ch] + eps));
    stats_w[ch] = mean;
    stats_w[NCH + ch] = invstd;
    stats_w[2 * NCH + ch] = mean_var[NCH + ch];
  } else {
    mean = stats_r[ch];
    invstd = stats_r[NCH + ch];
  }
  make_ab(gamma[ch], bias[ch], mean, invstd, tab + WS_ALPHA + ch, tab + WS_BETA + ch);
}

// y = relu(c3 alpha + beta)
__global__ __launch_bounds__(HDN_BLOCK) void output_kernel(const float* __restrict__ c3, const float* __restrict__ tab, float* __restrict__ out, long long n) {
  const long long i = (long long)blockIdx.x * HDN_BLOCK + threadIdx.x;
  if (i < n) out[i] = fmaxf(__builtin_fmaf(c3[i], tab[WS_ALPHA + 12], tab[WS_BETA + 12]), 0.f);
}

// ---------------------------------------------------------------------------------------------------------------- backward
// dz = g [c alpha + beta > 0], x^ = (c - mean) invstd: the workgroup's sums of dz and dz x^ per channel, part[blk][2 co], part[blk][2 co + 1]
template <int CO>
__global__ __launch_bounds__(HDN_BLOCK) void bn_reduce_kernel(const float* __restrict__ g, const float* __restrict__ c, const float* __restrict__ tab,
                                                              const float* __restrict__ stats, int ch0, double* __restrict__ part, int HW, int nbx) {
  __shared__ double red[WAVES * 2 * CO];
  const int b = blockIdx.x / nbx, bx = blockIdx.x - b * nbx;
  const float* gb = g + size_t(b) * CO * HW;
  const float* cb = c + size_t(b) * CO * HW;
  double sums[2 * CO];
#pragma unroll
  for (int q = 0; q < 2 * CO; ++q) sums[q] = 0.0;
#pragma unroll 1
  for (int i = 0; i < PX; ++i) {
    const int pix = bx * PXB + i * HDN_BLOCK + threadIdx.x;
    if (pix >= HW) continue;
#pragma unroll
    for (int co = 0; co < CO; ++co) {
      const float cv = cb[size_t(co) * HW + pix];
      const float z = __builtin_fmaf(cv, tab[WS_ALPHA + ch0 + co], tab[WS_BETA + ch0 + co]);
      const float dz = z > 0.f ? gb[size_t(co) * HW + pix] : 0.f;
      const float xh = rn_mul(rn_sub(cv, stats[ch0 + co]), stats[NCH + ch0 + co]);
      sums[2 * co] += (double)dz;
      sums[2 * co + 1] += (double)dz * (double)xh;
    }
  }
  block_sum_store<2 * CO, WAVES>(sums, red, part + size_t(blockIdx.x) * 2 * CO);
}

// one workgroup: S1, S2 of CO channels into the table (for the apply launch) and, gpar != NULL, into grad_bias / grad_gamma
__global__ __launch_bounds__(HDN_BLOCK) void bn_finish_kernel(const double* __restrict__ part, int nblk, int CO, int ch0, float* __restrict__ tab,
                                                              float* __restrict__ gpar) {
  __shared__ double red[WAVES];
  for (int co = 0; co < CO; ++co) {
    const double s1 = block_total(part + 2 * co, nblk, 2 * CO, red);
    const double s2 = block_total(part + 2 * co + 1, nblk, 2 * CO, red);
    if (threadIdx.x == 0) {
      const int ch = ch0 + co;
      tab[WS_S1 + ch] = (float)s1;
      tab[WS_S2 + ch] = (float)s2;
      if (gpar) {
        gpar[396 + ch] = (float)s2;       // grad_gamma
        gpar[396 + NCH + ch] = (float)s1;  // grad_bias
      }
    }
  }
}

// dc = alpha (dz - S1 / N - x^ S2 / N) with batch statistics, alpha dz with frozen ones (inv_n = 0 selects it: the statistics are constants then)
template <int CO>
__global__ __launch_bounds__(HDN_BLOCK) void bn_apply_kernel(const float* __restrict__ g, const float* __restrict__ c, const float* __restrict__ tab,
                                                             const float* __restrict__ stats, int ch0, float inv_n, int batch, float* __restrict__ dc,
                                                             int HW, long long n) {
  const long long i = (long long)blockIdx.x * HDN_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int co = (int)((i / HW) % CO), ch = ch0 + co;
  const float cv = c[i], alpha = tab[WS_ALPHA + ch];
  const float z = __builtin_fmaf(cv, alpha, tab[WS_BETA + ch]);
  const float dz = z > 0.f ? g[i] : 0.f;
  float v = dz;
  if (batch) {
    const float xh = rn_mul(rn_sub(cv, stats[ch]), stats[NCH + ch]);
    v = rn_sub(rn_sub(dz, rn_mul(tab[WS_S1 + ch], inv_n)), rn_mul(xh, rn_mul(tab[WS_S2 + ch], inv_n)));
  }
  dc[i] = rn_mul(alpha, v);
}

// the convolution's data adjoint as a gather: ga[b][ci](p) = sum over co, k of w[co][ci][k] dc[b][co](p - k)
template <int CI, int CO>
__global__ __launch_bounds__(HDN_BLOCK) void conv_data_adjoint_kernel(const float* __restrict__ dc, const float* __restrict__ w, float* __restrict__ ga,
                                                                      int H, int W, int nbx) {
  const int b = blockIdx.x / nbx, bx = blockIdx.x - b * nbx;
  const int HW = H * W;
  const float* db = dc + size_t(b) * CO * HW;
  float* gb = ga + size_t(b) * CI * HW;
#pragma unroll 1
  for (int i = 0; i < PX; ++i) {
    const int pix = bx * PXB + i * HDN_BLOCK + threadIdx.x;
    if (pix >= HW) continue;
    const int y = pix / W, x = pix - y * W;
    float acc[CI];
#pragma unroll
    for (int ci = 0; ci < CI; ++ci) acc[ci] = 0.f;
#pragma unroll
    for (int co = 0; co < CO; ++co) {
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const int yy = y - (k / 3 - 1), xx = x - (k % 3 - 1);
        const float d = ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) ? db[size_t(co) * HW + yy * W + xx] : 0.f;
#pragma unroll
        for (int ci = 0; ci < CI; ++ci) acc[ci] = __builtin_fmaf(w[(co * CI + ci) * 9 + k], d, acc[ci]);
      }
    }
#pragma unroll
    for (int ci = 0; ci < CI; ++ci) gb[size_t(ci) * HW + pix] = acc[ci];
  }
}

// the convolution's weight adjoint, input channel ci = blockIdx.y: the workgroup's sums of dc[co](p) a[ci](p + k), part[((co CI + ci) 9 + k) nblk + blk]
template <int CI, int CO, bool FIRST>
__global__ __launch_bounds__(HDN_BLOCK) void conv_weight_adjoint_kernel(const float* __restrict__ dc, const float* __restrict__ in,
                                                                        const float* __restrict__ tab, float* __restrict__ part, int H, int W, int nbx) {
  __shared__ float red[WAVES * CO * 9];
  const int b = blockIdx.x / nbx, bx = blockIdx.x - b * nbx;
  const int ci = blockIdx.y;
  const int HW = H * W;
  const float* db = dc + size_t(b) * CO * HW;
  const float* ip = in + (size_t(b) * CI + ci) * HW;
  const float alpha = FIRST ? 1.f : tab[WS_ALPHA + ci], beta = FIRST ? 0.f : tab[WS_BETA + ci];
  float acc[CO * 9];
#pragma unroll
  for (int q = 0; q < CO * 9; ++q) acc[q] = 0.f;
#pragma unroll 1
  for (int i = 0; i < PX; ++i) {
    const int pix = bx * PXB + i * HDN_BLOCK + threadIdx.x;
    if (pix >= HW) continue;
    const int y = pix / W, x = pix - y * W;
    float a[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) a[k] = act_at<FIRST>(ip, y + k / 3 - 1, x + k % 3 - 1, H, W, alpha, beta);
#pragma unroll
    for (int co = 0; co < CO; ++co) {
      const float d = db[size_t(co) * HW + pix];
#pragma unroll
      for (int k = 0; k < 9; ++k) acc[co * 9 + k] = __builtin_fmaf(d, a[k], acc[co * 9 + k]);
    }
  }
  // block_sum_store's order with the store spelled out: thread q = co 9 + k owns weight (co, ci, k), whose place (co CI 9 + ci 9 + k) nblk + blk
  // is no base + q stride once CI > 1
  const int nblk = gridDim.x, tid = threadIdx.x;
#pragma unroll
  for (int q = 0; q < CO * 9; ++q) acc[q] = wave_sum(acc[q]);
  if (lane_id() == 0) {
#pragma unroll
    for (int q = 0; q < CO * 9; ++q) red[wave_id() * CO * 9 + q] = acc[q];
  }
  __syncthreads();
  if (tid < CO * 9) {
    float s = red[tid];
#pragma unroll
    for (int wv = 1; wv < WAVES; ++wv) s = rn_add(s, red[wv * CO * 9 + tid]);
    const int co = tid / 9, k = tid - co * 9;
    part[size_t((co * CI + ci) * 9 + k) * nblk + blockIdx.x] = s;
  }
}

// one wave per weight: its nblk partials added in a fixed order, in float64, rounded once
__global__ __launch_bounds__(HDN_WAVE) void weight_finish_kernel(const float* __restrict__ part, int nblk, float* __restrict__ gw) {
  const float* p = part + size_t(blockIdx.x) * nblk;
  double s = 0.0;
  for (int k = threadIdx.x; k < nblk; k += HDN_WAVE) s += (double)p[k];
  s = wave_sum(s);
  if (threadIdx.x == 0) gw[blockIdx.x] = (float)s;
}

// ---------------------------------------------------------------------------------------------------------------- host
static int check_shape(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return HDN_E_SHAPE;
  if ((long long)B * H * W * NCH > 0x7fffffffLL) return HDN_E_LIMIT;
  return HDN_OK;
}

}  // namespace sft
}  // namespace hdn

extern "C" {

long long hdn_share_feature_train_saved_bytes(int B, int H, int W) {
  const int rc = hdn::sft::check_shape(B, H, W);
  if (rc) return rc;
  return (long long)B * H * W * hdn::sft::NCH * sizeof(float);
}

long long hdn_share_feature_train_workspace_bytes(int B, int H, int W) {
  using namespace hdn::sft;
  const int rc = check_shape(B, H, W);
  if (rc) return rc;
  const long long nblk = (long long)B * hdn::cdiv(H * W, PXB);
  return (WS_HEAD + nblk * PART_FLOATS + 16LL * B * H * W) * (long long)sizeof(float);
}

int hdn_share_feature_train_fwd_f32(const float* img, const float* w1, const float* w2, const float* w3, const float* gamma, const float* bias,
                                    const float* mean_var_or_null, float eps1, float eps2, float eps3, int stats_mode, float* out, float* saved,
                                    float* stats_out, float* workspace, long long workspace_bytes, int B, int H, int W, void* stream) {
  using namespace hdn;
  using namespace hdn::sft;
  if (!img || !w1 || !w2 || !w3 || !gamma || !bias || !out || !saved || !stats_out || !workspace) return HDN_E_NULL;
  if (stats_mode != 0 && stats_mode != 1) return HDN_E_SHAPE;
  if (stats_mode == 1 && !mean_var_or_null) return HDN_E_NULL;
  int rc = check_shape(B, H, W);
  if (rc == HDN_OK && stats_mode == 0 && (long long)B * H * W < 2) rc = HDN_E_SHAPE;
  if (rc) return rc;
  const long long need = hdn_share_feature_train_workspace_bytes(B, H, W);
  if (!aligned16(workspace) || workspace_bytes < need) return HDN_E_LIMIT;
  const long long n = (long long)B * H * W;
  const Range r[11] = {{out, n * 4},  {saved, n * NCH * 4}, {stats_out, 3 * NCH * 4}, {workspace, need}, {img, n * 4},
                       {w1, 36 * 4},  {w2, 288 * 4},        {w3, 72 * 4},             {gamma, NCH * 4},  {bias, NCH * 4},
                       {stats_mode == 1 ? mean_var_or_null : nullptr, 2 * NCH * 4}};
  if (any_output_overlaps(r, 4, 11)) return HDN_E_ALIAS;

  hipStream_t st = static_cast<hipStream_t>(stream);
  const int nbx = cdiv(H * W, PXB), nblk = B * nbx;
  float* tab = workspace;
  double* part = stats_mode == 0 ? reinterpret_cast<double*>(workspace + WS_HEAD) : nullptr;
  float *c1 = saved, *c2 = saved + 4 * n, *c3 = saved + 12 * n;
  const double N = (double)n;
  if (stats_mode == 1)
    hipLaunchKernelGGL(table_kernel, dim3(1), dim3(HDN_WAVE), 0, st, mean_var_or_null, eps1, eps2, eps3, gamma, bias, stats_out,
                       (const float*)nullptr, tab);
  hipLaunchKernelGGL((conv_stats_kernel<1, 4, true>), dim3(nblk), dim3(HDN_BLOCK), 0, st, img, w1, (const float*)tab, c1, part, H, W, nbx);
  if (part) hipLaunchKernelGGL(stats_finish_kernel, dim3(1), dim3(HDN_BLOCK), 0, st, (const double*)part, nblk, 4, 0, N, (double)eps1, gamma, bias, stats_out, tab);
  hipLaunchKernelGGL((conv_stats_kernel<4, 8, false>), dim3(nblk), dim3(HDN_BLOCK), 0, st, (const float*)c1, w2, (const float*)tab, c2, part, H, W, nbx);
  if (part) hipLaunchKernelGGL(stats_finish_kernel, dim3(1), dim3(HDN_BLOCK), 0, st, (const double*)part, nblk, 8, 4, N, (double)eps2, gamma, bias, stats_out, tab);
  hipLaunchKernelGGL((conv_stats_kernel<8, 1, false>), dim3(nblk), dim3(HDN_BLOCK), 0, st, (const float*)c2, w3, (const float*)(tab + 4), c3, part, H, W, nbx);
  if (part) hipLaunchKernelGGL(stats_finish_kernel, dim3(1), dim3(HDN_BLOCK), 0, st, (const double*)part, nblk, 1, 12, N, (double)eps3, gamma, bias, stats_out, tab);
  hipLaunchKernelGGL(output_kernel, dim3((unsigned)((n + HDN_BLOCK - 1) / HDN_BLOCK)), dim3(HDN_BLOCK), 0, st, (const float*)c3, (const float*)tab, out, n);
  return launch_status();
}

int hdn_share_feature_bwd_f32(const float* img, const float* w1, const float* w2, const float* w3, const float* gamma, const float* bias,
                              const float* saved, const float* stats, const float* grad_out, float* grad_img_or_null, float* grad_params_or_null,
                              float* workspace, long long workspace_bytes, int stats_mode, int B, int H, int W, void* stream) {
  using namespace hdn;
  using namespace hdn::sft;
  if (!img || !w1 || !w2 || !w3 || !gamma || !bias || !saved || !stats || !grad_out || !workspace) return HDN_E_NULL;
  if ((stats_mode != 0 && stats_mode != 1) || (!grad_img_or_null && !grad_params_or_null)) return HDN_E_SHAPE;
  int rc = check_shape(B, H, W);
  if (rc == HDN_OK && stats_mode == 0 && (long long)B * H * W < 2) rc = HDN_E_SHAPE;
  if (rc) return rc;
  const long long need = hdn_share_feature_train_workspace_bytes(B, H, W);
  if (!aligned16(workspace) || workspace_bytes < need) return HDN_E_LIMIT;
  const long long n = (long long)B * H * W;
  const Range r[12] = {{grad_img_or_null, n * 4}, {grad_params_or_null, NPAR * 4}, {workspace, need}, {img, n * 4},         {w1, 36 * 4},
                       {w2, 288 * 4},             {w3, 72 * 4},                    {gamma, NCH * 4},  {bias, NCH * 4},      {saved, n * NCH * 4},
                       {stats, 3 * NCH * 4},      {grad_out, n * 4}};
  if (any_output_overlaps(r, 3, 12)) return HDN_E_ALIAS;

  hipStream_t st = static_cast<hipStream_t>(stream);
  const int HW = H * W, nbx = cdiv(HW, PXB), nblk = B * nbx;
  const int batch = stats_mode == 0;
  const float inv_n = (float)(1.0 / (double)n);
  float* tab = workspace;
  float* partf = workspace + WS_HEAD;
  double* partd = reinterpret_cast<double*>(partf);
  float* bufA = partf + (long long)nblk * PART_FLOATS;  // the gradient of a layer's activations (up to 8 planes)
  float* bufB = bufA + 8 * n;                           // dc of the layer at hand (up to 8 planes)
  const float *c1 = saved, *c2 = saved + 4 * n, *c3 = saved + 12 * n;
  float* gp = grad_params_or_null;
  const bool sums = batch || gp;  // S1 / S2 feed dc with batch statistics and are grad_bias / grad_gamma
  const auto eblocks = [](long long m) { return dim3((unsigned)((m + HDN_BLOCK - 1) / HDN_BLOCK)); };

  hipLaunchKernelGGL(table_kernel, dim3(1), dim3(HDN_WAVE), 0, st, (const float*)nullptr, 0.f, 0.f, 0.f, gamma, bias, (float*)nullptr, stats, tab);
  // layer 3: 8 -> 1
  if (sums) {
    hipLaunchKernelGGL(bn_reduce_kernel<1>, dim3(nblk), dim3(HDN_BLOCK), 0, st, grad_out, c3, (const float*)tab, stats, 12, partd, HW, nbx);
    hipLaunchKernelGGL(bn_finish_kernel, dim3(1), dim3(HDN_BLOCK), 0, st, (const double*)partd, nblk, 1, 12, tab, gp);
  }
  hipLaunchKernelGGL(bn_apply_kernel<1>, eblocks(n), dim3(HDN_BLOCK), 0, st, grad_out, c3, (const float*)tab, stats, 12, inv_n, batch, bufB, HW, n);
  if (gp) {
    hipLaunchKernelGGL((conv_weight_adjoint_kernel<8, 1, false>), dim3(nblk, 8), dim3(HDN_BLOCK), 0, st, (const float*)bufB, c2,
                       (const float*)(tab + 4), partf, H, W, nbx);
    hipLaunchKernelGGL(weight_finish_kernel, dim3(72), dim3(HDN_WAVE), 0, st, (const float*)partf, nblk, gp + 324);
  }
  hipLaunchKernelGGL((conv_data_adjoint_kernel<8, 1>), dim3(nblk), dim3(HDN_BLOCK), 0, st, (const float*)bufB, w3, bufA, H, W, nbx);
  // layer 2: 4 -> 8
  if (sums) {
    hipLaunchKernelGGL(bn_reduce_kernel<8>, dim3(nblk), dim3(HDN_BLOCK), 0, st, (const float*)bufA, c2, (const float*)tab, stats, 4, partd, HW, nbx);
    hipLaunchKernelGGL(bn_finish_kernel, dim3(1), dim3(HDN_BLOCK), 0, st, (const double*)partd, nblk, 8, 4, tab, gp);
  }
  hipLaunchKernelGGL(bn_apply_kernel<8>, eblocks(8 * n), dim3(HDN_BLOCK), 0, st, (const float*)bufA, c2, (const float*)tab, stats, 4, inv_n, batch, bufB,
                     HW, 8 * n);
  if (gp) {
    hipLaunchKernelGGL((conv_weight_adjoint_kernel<4, 8, false>), dim3(nblk, 4), dim3(HDN_BLOCK), 0, st, (const float*)bufB, c1, (const float*)tab,
                       partf, H, W, nbx);
    hipLaunchKernelGGL(weight_finish_kernel, dim3(288), dim3(HDN_WAVE), 0, st, (const float*)partf, nblk, gp + 36);
  }
  hipLaunchKernelGGL((conv_data_adjoint_kernel<4, 8>), dim3(nblk), dim3(HDN_BLOCK), 0, st, (const float*)bufB, w2, bufA, H, W, nbx);
  // layer 1: 1 -> 4
  if (sums) {
    hipLaunchKernelGGL(bn_reduce_kernel<4>, dim3(nblk), dim3(HDN_BLOCK), 0, st, (const float*)bufA, c1, (const float*)tab, stats, 0, partd, HW, nbx);
    hipLaunchKernelGGL(bn_finish_kernel, dim3(1), dim3(HDN_BLOCK), 0, st, (const double*)partd, nblk, 4, 0, tab, gp);
  }
  if (gp || grad_img_or_null)
    hipLaunchKernelGGL(bn_apply_kernel<4>, eblocks(4 * n), dim3(HDN_BLOCK), 0, st, (const float*)bufA, c1, (const float*)tab, stats, 0, inv_n, batch,
                       bufB, HW, 4 * n);
  if (gp) {
    hipLaunchKernelGGL((conv_weight_adjoint_kernel<1, 4, true>), dim3(nblk, 1), dim3(HDN_BLOCK), 0, st, (const float*)bufB, img, (const float*)tab,
                       partf, H, W, nbx);
    hipLaunchKernelGGL(weight_finish_kernel, dim3(36), dim3(HDN_WAVE), 0, st, (const float*)partf, nblk, gp);
  }
  if (grad_img_or_null)
    hipLaunchKernelGGL((conv_data_adjoint_kernel<1, 4>), dim3(nblk), dim3(HDN_BLOCK), 0, st, (const float*)bufB, w1, grad_img_or_null, H, W, nbx);
  return launch_status();
}

}  // extern "C"
