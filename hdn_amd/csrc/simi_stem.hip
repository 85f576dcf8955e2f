// simi_stem.hip — the first stage of the similarity branch's ResNet-50 (stride 8, atrous) in one launch, on the matrix cores:
//   out[B,Sp,Sp,64] = maxpool3x3/s2/p1( relu( conv7x7/s2/p0(x[B,3,S,S], w[64][3][7][7]) + bias ) ),   Sc = (S - 7) / 2 + 1,  Sp = (Sc - 1) / 2 + 1
//   x NCHW fp32 (what the crop kernels hand the model), out channels-last fp32 (what layer1's hdn_conv1x1_f32 takes); 255 -> 125 -> 63, 127 -> 61 -> 31.
// Reference: ResNet.forward, hdn/models/backbone/resnet_atrous.py:117-121, 186-189 (conv1 / bn1 / relu / maxpool; eval mode, BatchNorm folded into
// (w, bias) by the caller).  Replaces four launches of the level-1 HIP backbone (MIOpen convolution, hdn_bias_relu_f32, max pool, NCHW -> channels-last
// copy); the Sc x Sc x 64 convolution map never goes to HBM.
//
// Arithmetic: trunk_stem_mfma.hip's implicit GEMM, D[conv pixel][co] = sum over k of A[pixel][k] W[k][co] on v_mfma_f32_32x32x16_f16, fp32 carried as
// two fp16 pieces (activations split as x 2^-8: pixel values of 0..255 scale are exact in the first piece), three piece products into hi / lo
// accumulators (mfma_split.h).  K = 3 x 7 x 8 = 168 (kx padded to 8 with a zero weight) in 11 k steps:
//   k = 16 step + 8 g + j  <->  row r = 2 step + g = ci * 7 + ky,  kx = j;   r = 21 (step 10, g = 1) and j = 7 are zero weights,
// so an A fragment (lane = (conv column, k half g), 8 consecutive k) is EIGHT CONSECUTIVE INPUT PIXELS of one input row, starting at input column
// 2 ox (stride 2, no left padding).  Summation order of a conv output: k steps 0 .. 10 into zeroed accumulators, join, + bias — the same whichever
// workgroup computes it and whatever B is, so an image gives the same bits at any batch size and in any call.
//
// Workgroup geometry: 256 threads = 4 waves; workgroup = (image b, pooled row p, channel half h), grid = B x Sp x 2 (B = 1: 126 workgroups at 255 px,
// 62 at 127 px).  It computes the three conv rows 2p - 1, 2p, 2p + 1 of its pooled row for its 32 channels (a conv row with an odd index is computed by
// two workgroups, with identical operations).  Wave ct owns MFMA row tile ct: tile row i = 32 ct + li is conv column i - 1, so that the pool's left
// neighbour (column 2 px - 1) lives in the same row of tiles: pooled column px reads i = 2 px, 2 px + 1, 2 px + 2.  i <= 127 and 2 (Sp - 1) + 2 <= 127
// give the size limit Sc <= 126; the entry point documents and enforces S <= MAX_S = 255 (Sc <= 125).
//   1. the 11 input rows 4p - 2 .. 4p + 8 of the three channels are split ONCE into the two fp16 pieces while they are staged in LDS
//      ([ci][piece][11 rows][PITCH dwords]; staged column 2 + (input column), zeros outside the image); an A fragment is then 16 bytes at the
//      4-byte-aligned address row + 4 i.  PITCH = 160 dwords: the two k halves of a wave (consecutive rows) sit 32 banks apart.
//      This half's weights (host-packed in fragment order, 22.5 KB) are copied to LDS beside them.
//   2. 11 k steps x 3 conv rows x 3 MFMAs per wave (a wave whose tile lies right of the image skips them).
//   3. join + bias + ReLU; conv rows / columns outside the map become 0 (behind the ReLU everything is >= 0 and every pool window holds a real element,
//      so the pool's -inf padding is a plain skip); the vertical max of the three rows stays in registers (same lane, same register of the three
//      accumulators) and goes to LDS as [128 tile rows][32 channels] fp32 (over the staged input, after a barrier);
//   4. the horizontal max of three LDS rows per pooled column, written as 128-byte channel runs.
// LDS: 42,240 (input) + 22,528 (weights) = 64,768 bytes: two workgroups per CU.
#include "hdn_common.h"
#include "mfma_split.h"

namespace hdn {
namespace simi_stem {
using namespace hdn::mc;

constexpr int CO = 64, CIN = 3, NSTEP = 11, NR = 21;           // NR = 3 x 7 (ci, ky) rows of K
constexpr int MAX_S = 255;
constexpr int ROWS = 11;                                       // input rows of three conv rows
constexpr int PITCH = 160;                                     // dwords (fp16 pairs) per staged row
constexpr int PAIRS = 132;                                     // staged pairs per row: dwords 0 .. 130 are read (i + 3, i <= 127)
constexpr int PIECE_BYTES = ROWS * PITCH * 4;
constexpr int A_BYTES = CIN * 2 * PIECE_BYTES;                 // [ci][piece][row][PITCH]
constexpr int W_WORDS = NSTEP * 2 * 64;                        // 16-byte words of one channel half: [k step][piece][lane]
constexpr int W_BYTES = W_WORDS * 16;
constexpr int LDS_BYTES = A_BYTES + W_BYTES;
constexpr int ITEMS = CIN * ROWS * PAIRS;
constexpr int THREADS = 256;
static_assert(128 * 32 * 4 <= A_BYTES, "the pool buffer reuses the staged input");
static_assert(127 + 3 < PAIRS && PAIRS <= PITCH, "staged row: tile row i reads dwords i .. i + 3");

struct __attribute__((packed, aligned(4))) Frag {              // 8 halves at a 4-byte-aligned LDS address
  unsigned d[4];
};

__device__ __forceinline__ float max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

__global__ __launch_bounds__(THREADS) void simi_stem_kernel(const float* __restrict__ x, const u32x4* __restrict__ wfrag, const float* __restrict__ bias,
                                                            float* __restrict__ out, int S, int Sc, int Sp) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* const sA = smem;
  u32x4* const sW = reinterpret_cast<u32x4*>(smem + A_BYTES);
  float* const sP = reinterpret_cast<float*>(smem);            // [128][32], after the MFMAs
  const int tid = threadIdx.x, lane = tid & 63;
  const int ct = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, g = lane >> 5;
  const int h = blockIdx.x & 1, bp = blockIdx.x >> 1, b = bp / Sp, p = bp - b * Sp;
  const float* const xb = x + (size_t)b * CIN * S * S;

  // ---- 1. this half's weights -> LDS; input rows 4p - 2 .. 4p + 8 -> fp16 pieces in LDS (every load in flight before the first use)
  for (int i = tid; i < W_WORDS; i += THREADS) {
    const int s = i >> 7, rest = i & 127;                      // [k step][piece][lane] <- [k step][n tile h][piece][lane]
    sW[i] = wfrag[(s * 2 + h) * 128 + rest];
  }
  {
    constexpr int NIT = cdiv(ITEMS, THREADS);
    f2 v[NIT];
    const int y_lo = 4 * p - 2;
#pragma unroll
    for (int k = 0; k < NIT; ++k) {
      const int item = min(tid + k * THREADS, ITEMS - 1);
      const int pr = item % PAIRS, rc = item / PAIRS, ci = rc / ROWS, y = y_lo + (rc - ci * ROWS);
      const int x0 = 2 * pr - 2;                               // image column of the pair's first element
      const float* src = xb + ((size_t)ci * S + min(max(y, 0), S - 1)) * S;
      const float a = src[min(max(x0, 0), S - 1)], c = src[min(max(x0 + 1, 0), S - 1)];
      const bool yin = y >= 0 && y < S;
      v[k] = f2{yin && x0 >= 0 && x0 < S ? a : 0.f, yin && x0 + 1 >= 0 && x0 + 1 < S ? c : 0.f};
    }
#pragma unroll
    for (int k = 0; k < NIT; ++k) {
      const int item = tid + k * THREADS;
      if (item < ITEMS) {
        const int pr = item % PAIRS, rc = item / PAIRS, ci = rc / ROWS, slot = rc - ci * ROWS;
        unsigned p0, p1;
        split2(v[k], p0, p1);
        unsigned char* dst = sA + (size_t)(ci * 2) * PIECE_BYTES + (slot * PITCH + pr) * 4;
        *reinterpret_cast<unsigned*>(dst) = p0;
        *reinterpret_cast<unsigned*>(dst + PIECE_BYTES) = p1;
      }
    }
  }
  const float bias_c = bias[32 * h + li];                      // C / D layout: column (channel) = lane & 31
  __syncthreads();

  // ---- 2. conv rows 2p - 1 + cr, cr = 0 .. 2: input row slot of tap ky = 2 cr + ky
  f32x16 hi[3], lo[3];
#pragma unroll
  for (int cr = 0; cr < 3; ++cr)
#pragma unroll
    for (int r = 0; r < 16; ++r) hi[cr][r] = lo[cr][r] = 0.f;
  if (32 * ct - 1 < Sc) {                                      // (wave-uniform) the tile's first conv column is inside the map
    const unsigned char* const a_lane = sA + 4 * (32 * ct + li);
    static_for<NSTEP>([&](auto Sn) {
      constexpr int s = decltype(Sn)::value;
      constexpr int r0 = 2 * s, r1 = 2 * s + 1 < NR ? 2 * s + 1 : NR - 1;        // r = 21: zero weights; any finite row will do
      constexpr int o0 = ((r0 / 7) * 2 * ROWS + (r0 % 7)) * PITCH * 4, o1 = ((r1 / 7) * 2 * ROWS + (r1 % 7)) * PITCH * 4;
      const unsigned char* const pa = a_lane + (g ? o1 : o0);
      u32x4 a[3][2], bf[2];
#pragma unroll
      for (int cr = 0; cr < 3; ++cr)
#pragma unroll
        for (int pc = 0; pc < 2; ++pc) {
          const Frag f = *reinterpret_cast<const Frag*>(pa + pc * PIECE_BYTES + 2 * cr * PITCH * 4);
          a[cr][pc] = u32x4{f.d[0], f.d[1], f.d[2], f.d[3]};
        }
#pragma unroll
      for (int pc = 0; pc < 2; ++pc) bf[pc] = sW[(s * 2 + pc) * 64 + lane];
#pragma unroll
      for (int cr = 0; cr < 3; ++cr) lo[cr] = mfma(a[cr][1], bf[0], lo[cr]);
#pragma unroll
      for (int cr = 0; cr < 3; ++cr) hi[cr] = mfma(a[cr][0], bf[0], hi[cr]);
#pragma unroll
      for (int cr = 0; cr < 3; ++cr) lo[cr] = mfma(a[cr][0], bf[1], lo[cr]);
    });
  }
  __syncthreads();                                             // every wave is done with the staged input: sP may overwrite it

  // ---- 3. relu(conv + bias), 0 outside the map, vertical max -> sP[tile row i][channel]
  bool rin[3];
#pragma unroll
  for (int cr = 0; cr < 3; ++cr) rin[cr] = 2 * p - 1 + cr >= 0 && 2 * p - 1 + cr < Sc;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = 32 * ct + d_row(r, g), col = i - 1;
    float m = 0.f;
#pragma unroll
    for (int cr = 0; cr < 3; ++cr) {
      const float c = fmaxf(join(hi[cr][r], lo[cr][r]) + bias_c, 0.f);
      m = fmaxf(m, rin[cr] ? c : 0.f);
    }
    sP[i * 32 + li] = (col >= 0 && col < Sc) ? m : 0.f;
  }
  __syncthreads();

  // ---- 4. pooled column px = max over tile rows 2 px .. 2 px + 2
  float* const orow = out + ((size_t)b * Sp + p) * Sp * CO + 32 * h;
  for (int idx = tid; idx < Sp * 32; idx += THREADS) {
    const int px = idx >> 5, c = idx & 31;
    const float* q = sP + (2 * px) * 32 + c;
    orow[(size_t)px * CO + c] = max3(q[0], q[32], q[64]);
  }
}

}  // namespace simi_stem
}  // namespace hdn

// wpacked (hdn_pack_simi_stem_f32): [11 k steps][2 n tiles][2 pieces][64 lanes = k half g x 32 + n][8] fp16: element j of lane (g, n) of k step s is
// piece pc of w[co = 32 tile + n][ci][ky][kx = j] with ci * 7 + ky = 2 s + g; 0 for j = 7 and for 2 s + g = 21.
extern "C" int hdn_simi_stem_f32(const float* x, const void* wpacked, const float* bias, float* out, int B, int S, int act_domain, void* stream) {
  using namespace hdn::simi_stem;
  if (!x || !wpacked || !bias || !out) return HDN_E_NULL;
  if (B <= 0 || S < 7 || act_domain != 0) return HDN_E_SHAPE;
  if (S > MAX_S) return HDN_E_LIMIT;
  const int Sc = (S - 7) / 2 + 1, Sp = (Sc - 1) / 2 + 1;
  const long long nx = (long long)B * CIN * S * S, nout = (long long)B * Sp * Sp * CO;
  if (nx > INT32_MAX || 2LL * B * Sp > INT32_MAX) return HDN_E_LIMIT;
  if (hdn::bytes_overlap(out, nout * 4, x, nx * 4)) return HDN_E_ALIAS;
  if (!hdn::aligned16(wpacked) || !hdn::aligned16(out)) return HDN_E_LIMIT;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (const int rc = hdn::check_fp16_range(x, nx, st)) return rc;
  static hdn::PerDeviceOnce attr;
  if (const int rc = hdn::lds_opt_in(attr, LDS_BYTES, &simi_stem_kernel)) return rc;
  hipLaunchKernelGGL(simi_stem_kernel, dim3((unsigned)(2 * B * Sp)), dim3(THREADS), LDS_BYTES, st, x, static_cast<const u32x4*>(wpacked), bias, out, S, Sc,
                     Sp);
  return hdn::launch_status();
}
