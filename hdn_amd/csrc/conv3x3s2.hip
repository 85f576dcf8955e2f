// The trunk's three stride-2 stages at large batches (round 5): relu(conv3x3/s2/p1(x, w) + b) AND the block's 1x1/s2 downsample branch from one
// staged input, on the matrix cores, in the producer / consumer form of conv3x3_v2_kernel (conv3x3.hip):
//   x [B, 2S, 2S, C] (channels-last) -> out [B, S, S, 2C] = relu(conv + bias),  out_ds [B, S, S, 2C] = the raw 1x1 / stride-2 product
// Reference: BasicBlock.forward with a downsample branch, homo_estimator/Deep_homography/Oneline_DLTv1/backbone/resnet.py:78-94 (conv1 + bn1 + relu
// and downsample(x); BatchNorm folded into the weights, the branch's bias goes to the block's second convolution: hdn_amd.trunk.FusedBasicBlock).
// hdn_conv3x3s2_ds_f32 (conv3x3.hip, round 4) stays the form for small batches.
//
// fp32 as two fp16 pieces (x = h0 + 2^-11 h1), three piece products into hi / lo accumulators: the error of an fp32 convolution (conv3x3.hip).
// Workgroup = 64 output pixels x 64 output channels: 4 producer waves + 4 consumer waves.  The producers stage the (2R + 1) x (2S + 1) input patch of a
// chunk of 32 input channels as the two pieces' LDS images ([piece][k step][k half][pixel slot] x 16 B, double-buffered) and own the epilogue.  In an
// image row the EVEN padded columns come first, then the odd ones: the 32 pixels of an MFMA tile (consecutive output columns) read consecutive 16-byte
// slots for every tap - (ky, kx) is a constant of the ds_read's offset field: (ky * PW + {0, PWH, 1}[kx]) * 16 - instead of every other one.
// Consumer wave = (pixel half wm, k step wk of the chunk): a 32 x 64 output tile, ten steps per chunk - the nine taps and, with the centre tap's fragment
// again, the downsample branch's weights into a second pair of accumulators.  The weights never touch the LDS: host-packed in fragment order, they travel
// L2 -> registers four steps ahead.  The two k steps' partial tiles meet in LDS (over the dead images) and the producers write both outputs.
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "conv3x3_tile.h"
#include "hdn_common.h"
#include "mfma_split.h"

// Measurement hooks (tools/build_variant.sh ... -DHDN_ABLATION -D<experiment>): every site below expands to its production text; the
// experiments' replacement bodies live in ablation/conv3x3s2.inc and are compiled in only under -DHDN_ABLATION, so that editing or adding an
// experiment leaves this translation unit's text (and the hash the committed PMC record carries) unchanged.
#define HDN_ABL_CONV3X3S2_0(...) __VA_ARGS__
#define HDN_ABL_CONV3X3S2_1(...) __VA_ARGS__
#define HDN_ABL_CONV3X3S2_2(...) __VA_ARGS__
#define HDN_ABL_CONV3X3S2_3(...) __VA_ARGS__
#define HDN_ABL_CONV3X3S2_4(...) __VA_ARGS__
#define HDN_ABL_CONV3X3S2_5(...) __VA_ARGS__
#ifdef HDN_ABLATION
#include "ablation/conv3x3s2.inc"
#endif

namespace hdn {
namespace s2 {
using namespace hdn::mc;

// The LDS image of both kernels of this file: a chunk of 16 KS input channels of the (2R + 1) x (2 SO + 1) input patch of a tile of 64 output pixels,
// as [piece][k step][k half][pixel slot] x 16 B, the even padded columns of a row before the odd ones.
template <int SO_, int KS_>
struct Image {
  static constexpr int SO = SO_, SI = 2 * SO_, KS = KS_, BM = 64, BN = 64;
  static constexpr int IMGS = BM > SO * SO ? BM / (SO * SO) : 1;     // images per tile (4 x 4 outputs: four)
  static constexpr int R = BM / (SO * IMGS);                         // output rows of an image in the tile
  static constexpr int PH = 2 * R + 1;                               // padded input rows (one row of padding above, none needed below)
  static constexpr int NE = SO + 1, NO = SO, PWH = NE;               // even / odd padded columns of a row; slot of the first odd one
  // row pitch in slots: 16 lanes of a ds_read_b128 pass = 16 / SO rows of the MFMA tile, 2 PW slots apart - distinct bank groups for PW = 4 mod 8
  // (two rows of 8) and PW = 2 mod 8 (four rows of 4)
  static constexpr int PW = SO == 16 ? 33 : SO == 8 ? 20 : 10;
  static_assert(PW >= NE + NO, "row pitch");
  static constexpr int IPITCH = PH * PW, LPV = IMGS * IPITCH;
  static constexpr int LP = LPV + (4 - LPV % 16 + 16) % 16;          // = 4 mod 16: the four k groups a staging pass writes land on distinct banks
  static constexpr int KG_BYTES = LP * 16, KSTEP_BYTES = 2 * KG_BYTES, PIECE_BYTES = KS * KSTEP_BYTES, A_BYTES = 2 * PIECE_BYTES;
  static constexpr int EPI_STRIDE = epi_stride(BN);
  // byte offset in an image of tile pixel p's tap (0, 0) = padded (2 yy, 2 xx), k half g (MFMA row = lane & 31: p = 32 x the wave's pixel half + li)
  static __device__ __forceinline__ int aoff(int p, int g) {
    const int img = p / (R * SO), yy = (p / SO) % R, xx = p % SO;
    return g * KG_BYTES + (img * IPITCH + 2 * yy * PW + xx) * 16;
  }
};

// HDN_BLOCK threads stage a chunk: global -> registers (load_a) -> split -> image (store_a).  An item = (pixel slot, 8-channel group of the chunk): its
// source offset, validity and LDS address do not depend on the chunk and are worked out once (two divisions by constants per item and chunk otherwise:
// with producer waves, their instruction stream is what paces a chunk, not the loads' latency).  What the two kernels choose (Cf):
//   PAD_SLOTS  the items cover the LP - LPV padding slots as well (stored as zeros) and are addressed by item; otherwise by the (clamped) pixel slot
//   ASETS      register sets: a chunk's pixels may be asked for ASETS chunks before they are split
template <class Cf, bool SD>
struct Stager {
  static constexpr int KS = Cf::KS, AITEMS = (Cf::PAD_SLOTS ? Cf::LP : Cf::LPV) * 2 * KS, AITER = cdiv(AITEMS, HDN_BLOCK);
  using Set0 = std::integral_constant<int, 0>;
  uint32_t a_src[AITER], a_dst[AITER];
  bool a_ok[AITER];
  f4 av[Cf::ASETS][AITER][2];
  const int tid;

  // the tile's first image b0 and output row y0 of B images
  __device__ __forceinline__ Stager(int tid_, int b0, int y0, int B) : tid(tid_) {
#pragma unroll
    for (int q = 0; q < AITER; ++q) {
      const int item = tid + q * HDN_BLOCK, slot = item / (2 * KS), sub = item % (2 * KS);
      const int px = min(slot, Cf::LPV - 1);
      const int img = px / Cf::IPITCH, ry = (px % Cf::IPITCH) / Cf::PW, sl = px % Cf::IPITCH % Cf::PW;
      const int pc = sl < Cf::NE ? 2 * sl : 2 * (sl - Cf::NE) + 1;                 // padded column of the slot
      const int b = b0 + img, y = 2 * y0 + ry - 1, xx = pc - 1;
      a_ok[q] = item < AITEMS && (!Cf::PAD_SLOTS || slot < Cf::LPV) && sl < Cf::NE + Cf::NO && b < B && y >= 0 && y < Cf::SI && xx >= 0 && xx < Cf::SI;
      a_src[q] = a_ok[q] ? (uint32_t)(((b * Cf::SI + y) * Cf::SI + xx) * Cf::CI + sub * 8) : 0u;   // (floats; the whole input is < 2^31 of them)
      a_dst[q] = (uint32_t)(sub * Cf::KG_BYTES + (Cf::PAD_SLOTS ? slot : px) * 16);
    }
  }
  template <class SetC = Set0>
  __device__ __forceinline__ void load_a(const float* __restrict__ x, int chunk, SetC = {}) {
    HDN_ABL_CONV3X3S2_0()
#pragma unroll
    for (int q = 0; q < AITER; ++q) {
      const f4* src = reinterpret_cast<const f4*>(x + a_src[q] + chunk * (16 * KS));
      av[SetC::value][q][0] = a_ok[q] ? src[0] : f4{0.f, 0.f, 0.f, 0.f};
      av[SetC::value][q][1] = a_ok[q] ? src[1] : f4{0.f, 0.f, 0.f, 0.f};
    }
  }
  template <class SetC = Set0>
  __device__ __forceinline__ void store_a(unsigned char* image, SetC = {}) {
#pragma unroll
    for (int q = 0; q < AITER; ++q) {
      if (tid + q * HDN_BLOCK < AITEMS) split_store<Cf, SD>(av[SetC::value][q][0], av[SetC::value][q][1], image + a_dst[q]);
    }
  }
};

}  // namespace s2

namespace cvs {
using namespace hdn::mc;

template <int SO_, int CI_>
struct CfgS : s2::Image<SO_, 2> {
  using Img = s2::Image<SO_, 2>;
  static constexpr int CI = CI_, CO = 2 * CI_;
  static constexpr int NT = 2, WK = 2, WM = 2, NP = 2;
  static_assert(SO_ == 16 || SO_ == 8 || SO_ == 4, "the trunk's three stride-2 stages");
  static constexpr bool PAD_SLOTS = true;
  static constexpr int ASETS = 2;
  static constexpr int NCHUNK = CI / (16 * Img::KS), NB = CO / Img::BN;
  static constexpr int NS = 10;                                      // steps of a wave per chunk: nine taps + the downsample branch
  static constexpr int BSETS = 5, PF = BSETS - 1;                    // B register sets: a step's fragments travel PF steps ahead
  static_assert(NS % BSETS == 0 && NS % 2 == 0, "register sets rotate with the step");
  static constexpr int WSTEP = NT * NP * 64;                         // 16-byte words of one wave step: [n tile][piece][lane]
  static constexpr int WCHUNK = WK * NS * WSTEP;                     // ... of one (channel block, chunk): [k step][step]
  static constexpr int RED_FLOATS = WK * Img::BM * Img::EPI_STRIDE;  // one output's partial tiles
  static constexpr int RED_BYTES = 2 * RED_FLOATS * 4;
  static constexpr int LDS_BYTES = 2 * Img::A_BYTES > RED_BYTES ? 2 * Img::A_BYTES : RED_BYTES;
  static_assert(LDS_BYTES <= 160 * 1024 && 2 * Img::A_BYTES < 65536 * 2, "LDS");
};

template <class Cf, bool SD = false>
__global__ __launch_bounds__(2 * HDN_BLOCK) void conv3x3s2_v2_kernel(const float* __restrict__ x, const u32x4* __restrict__ wp, const float* __restrict__ bias,
                                                                 float* __restrict__ out, float* __restrict__ out_ds, int B) {
  constexpr int SO = Cf::SO, CO = Cf::CO, BM = Cf::BM, BN = Cf::BN, WK = Cf::WK, NS = Cf::NS, NT = Cf::NT, PF = Cf::PF;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x & (HDN_BLOCK - 1), lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool produce = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 8)) != 0;
  const int li = lane & 31, g = lane >> 5;
  const int nb = blockIdx.x;                                  // output-channel block, fastest: an XCD keeps its blocks' weight streams in its L2
  const long long M = (long long)B * SO * SO;
  const long long m0 = (long long)blockIdx.y * BM;
  const int b0 = (int)(m0 / (SO * SO)), y0 = (int)((m0 % (SO * SO)) / SO);
  float* const red = reinterpret_cast<float*>(smem);          // the partial tiles meet over the dead images

  if (produce) {
    // ------------------------------------------------------------------------------------------------ producers
    // two register sets: a chunk's pixels are asked for TWO chunks before they are split into the LDS image (a chunk is 10 steps of 6 MFMAs = under a
    // microsecond, less than a round trip to the previous launch's output).  Measured: no change against one set - what a chunk costs here is the
    // producers' own instruction stream (address arithmetic + 32 conversions per item, 6 items per thread: ablations in profiles/round5_conv3x3.txt)
    s2::Stager<Cf, SD> stager(tid, b0, y0, B);
    using S0 = std::integral_constant<int, 0>;
    using S1 = std::integral_constant<int, 1>;
    stager.load_a(x, 0, S0{});
    if (Cf::NCHUNK > 1) stager.load_a(x, 1, S1{});
    stager.store_a(smem, S0{});
    if (Cf::NCHUNK > 2) stager.load_a(x, 2, S0{});
    __syncthreads();                                   // chunk 0 is staged
    static_for<Cf::NCHUNK>([&](auto Cc) {              // chunk c + 1 -> its image (read last in chunk c - 1, one barrier ago); chunk c + 3 on its way
      constexpr int c = decltype(Cc)::value;
      using Set = std::integral_constant<int, (c + 1) & 1>;
      if constexpr (c + 1 < Cf::NCHUNK) {
        stager.store_a(smem + ((c + 1) & 1) * Cf::A_BYTES, Set{});
        if constexpr (c + 3 < Cf::NCHUNK) stager.load_a(x, c + 3, Set{});
      }
      __syncthreads();                                 // chunk c + 1 is staged; the consumers have read the last fragment of chunk c
    });
    __syncthreads();                                   // both outputs' partial tiles are in LDS
    // sum of the WK partial tiles in k order; the 3 x 3 output + bias, ReLU; the downsample branch raw.  A pixel's 64 channels = 16 consecutive lanes
    HDN_ABL_CONV3X3S2_1()
#pragma unroll
    for (int o = 0; o < 2; ++o) {
      const float* const rd = red + o * Cf::RED_FLOATS;
      float* const dst = o ? out_ds : out;
      for_tile_items<BM, BN, HDN_BLOCK>(tid, m0, M, [&](int, int px, int c4, long long m) {
        f4 v = *reinterpret_cast<const f4*>(rd + px * Cf::EPI_STRIDE + c4 * 4);
#pragma unroll
        for (int w = 1; w < WK; ++w) v = v + *reinterpret_cast<const f4*>(rd + (w * BM + px) * Cf::EPI_STRIDE + c4 * 4);
        if (o == 0) v = relu4(v + *reinterpret_cast<const f4*>(bias + nb * BN + c4 * 4));
        *reinterpret_cast<f4*>(dst + m * CO + nb * BN + c4 * 4) = v;
      });
    }
    return;
  }

  // -------------------------------------------------------------------------------------------------- consumers
  const int wm = wave / WK, wk = wave % WK;
  const uint32_t aoff = lds_addr(smem) + wk * Cf::KSTEP_BYTES + Cf::aoff(wm * 32 + li, g);   // this lane's A row, tap (0, 0), the wave's k step
  f32x16 acc[NT], accl[NT], dacc[NT], daccl[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[nt][r] = accl[nt][r] = dacc[nt][r] = daccl[nt][r] = 0.f;

  // this wave's weight stream: [channel block][chunk][k step][step][n tile][piece][lane] x 16 B
  const u32x4* const wbase = wp + (size_t)nb * Cf::NCHUNK * Cf::WCHUNK + (size_t)wk * NS * Cf::WSTEP;
  const uint32_t voff = (uint32_t)lane * 16u;
  u32x4 fb[Cf::BSETS][NT][2], fa[2][2];
  auto load_b = [&](u32x4 (&b)[NT][2], int ch, int st) {    // a step past the last chunk: the last step again (keeps the count of loads in flight static)
    HDN_ABL_CONV3X3S2_2()
    const bool past = ch >= Cf::NCHUNK;
    const u32x4* sp = wbase + (size_t)(past ? Cf::NCHUNK - 1 : ch) * Cf::WCHUNK + (size_t)(past ? NS - 1 : st) * Cf::WSTEP;
    asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(b[0][0]) : "v"(voff), "s"(sp));
    asm volatile("global_load_dwordx4 %0, %1, %2 offset:1024" : "=v"(b[0][1]) : "v"(voff), "s"(sp));
    asm volatile("global_load_dwordx4 %0, %1, %2 offset:2048" : "=v"(b[1][0]) : "v"(voff), "s"(sp));
    asm volatile("global_load_dwordx4 %0, %1, %2 offset:3072" : "=v"(b[1][1]) : "v"(voff), "s"(sp));
  };
  // A fragments of step ST (tap ST; step 9 = the downsample branch = the centre tap's fragment) from the image at `base`
  auto read_a = [&](u32x4 (&a)[2], uint32_t base, auto STc) {
    constexpr int ST = decltype(STc)::value, t = ST == 9 ? 4 : ST, ky = t / 3, kx = t % 3;
    constexpr int OFF = (ky * Cf::PW + (kx == 0 ? 0 : kx == 1 ? Cf::PWH : 1)) * 16;
    static_assert(OFF + Cf::PIECE_BYTES < 65536, "ds_read offset field");
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(a[0]) : "v"(base), "n"(OFF));
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(a[1]) : "v"(base), "n"(OFF + Cf::PIECE_BYTES));
  };
  using I0 = std::integral_constant<int, 0>;

  static_for<PF>([&](auto Ic) {                         // the first PF steps' fragments
    constexpr int i = decltype(Ic)::value;
    load_b(fb[i], i / NS, i % NS);
  });
  __builtin_amdgcn_s_barrier();                        // chunk 0 is staged
  read_a(fa[0], aoff, I0{});
  for (int chunk = 0; chunk < Cf::NCHUNK; ++chunk) {
    const uint32_t cur = aoff + (uint32_t)(chunk & 1) * Cf::A_BYTES, nxt = aoff + (uint32_t)((chunk + 1) & 1) * Cf::A_BYTES;
    static_for<NS>([&](auto Pc) {
      constexpr int st = decltype(Pc)::value, as = st % 2, bs = st % Cf::BSETS;
      {  // the B fragments PF steps ahead
        constexpr int q = st + PF;
        load_b(fb[(st + PF) % Cf::BSETS], chunk + q / NS, q % NS);
      }
      if constexpr (st + 1 < NS) {
        read_a(fa[as ^ 1], cur, std::integral_constant<int, st + 1>{});
        HDN_ABL_CONV3X3S2_3(asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(2)" ::"n"(PF * NT * 2) : "memory");)
      } else {
        HDN_ABL_CONV3X3S2_4(asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(PF * NT * 2) : "memory");)
        // the chunk's last fragments are in registers: the producers may overwrite its image, and the next chunk's image is complete
        __builtin_amdgcn_s_barrier();
        if (chunk + 1 < Cf::NCHUNK) read_a(fa[as ^ 1], nxt, I0{});
      }
#pragma unroll
      for (int pc = 0; pc < 2; ++pc) asm volatile("" : "+v"(fa[as][pc]));
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int pc = 0; pc < 2; ++pc) asm volatile("" : "+v"(fb[bs][nt][pc]));
      HDN_ABL_CONV3X3S2_5()
      if constexpr (st < 9) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) accl[nt] = mfma(fa[as][1], fb[bs][nt][0], accl[nt]);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = mfma(fa[as][0], fb[bs][nt][0], acc[nt]);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) accl[nt] = mfma(fa[as][0], fb[bs][nt][1], accl[nt]);
      } else {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) daccl[nt] = mfma(fa[as][1], fb[bs][nt][0], daccl[nt]);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) dacc[nt] = mfma(fa[as][0], fb[bs][nt][0], dacc[nt]);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) daccl[nt] = mfma(fa[as][0], fb[bs][nt][1], daccl[nt]);
      }
    });
  }
  // ---- this wave's two partial tiles -> LDS, over the images (every consumer has passed the last chunk's barrier after its last read).
  float* const rbase = red + (wk * BM + wm * 32 + 4 * g) * Cf::EPI_STRIDE + li;
  static_for<16>([&](auto Rc) {
    constexpr int r = decltype(Rc)::value, row = d_row(r);
    float* const q = rbase + row * Cf::EPI_STRIDE;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      q[nt * 32] = join<SD>(acc[nt][r], accl[nt][r]);
      q[Cf::RED_FLOATS + nt * 32] = join<SD>(dacc[nt][r], daccl[nt][r]);
    }
  });
  __syncthreads();                                     // the partial sums are in LDS (the producers take them from there)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // (the surplus B loads at the tail)
}

template <class Cf, bool SD = false>
static int launch(const float* x, const void* wp, const float* bias, float* out, float* out_ds, int B, hipStream_t stream) {
  const long long M = (long long)B * Cf::SO * Cf::SO;
  static PerDeviceOnce attr;
  if (const int rc = lds_opt_in(attr, Cf::LDS_BYTES, &conv3x3s2_v2_kernel<Cf, SD>)) return rc;
  if ((M + Cf::BM - 1) / Cf::BM > 65535) return HDN_E_LIMIT;      // grid.y (as launch_v2 of conv3x3.hip)
  const dim3 grid(Cf::NB, (unsigned)((M + Cf::BM - 1) / Cf::BM)), blk(2 * HDN_BLOCK);
  hipLaunchKernelGGL((conv3x3s2_v2_kernel<Cf, SD>), grid, blk, Cf::LDS_BYTES, stream, x, static_cast<const u32x4*>(wp), bias, out, out_ds, B);
  return launch_status();
}

}  // namespace cvs
}  // namespace hdn

// wpacked (hdn_amd.trunk.pack_conv3x3s2_ds_v2): [2C / 64][C / 32 chunks][2 k steps][10 steps][2 n tiles][2 pieces][k half g][n][8] fp16; element e of
// lane (g, n) of (block nb, chunk, k step wk, step t, n tile nt) = piece of w[co = 64 nb + 32 nt + n][ci = 32 chunk + 16 wk + 8 g + e][tap t] for
// t < 9 (t = 3 ky + kx), of the downsample branch's w_ds[co][ci] for t = 9.
extern "C" int hdn_conv3x3s2_v2_f32(const float* x, const void* wpacked, const float* bias, float* out, float* out_ds, int B, int S, int CI, int act_domain,
                                    void* stream) {
  if (B <= 0 || S <= 0 || CI <= 0 || (act_domain != 0 && act_domain != 1)) return HDN_E_SHAPE;
  if (!x || !wpacked || !bias || !out || !out_ds) return HDN_E_NULL;
  if (out == x || out_ds == x || out_ds == out) return HDN_E_ALIAS;
  const long long n_in = (long long)B * S * S * CI * 4;       // the input has 2S x 2S x CI elements = an output's count x 2
  if (n_in > 0x7fffffffLL) return HDN_E_LIMIT;
  for (const void* p : {(const void*)x, wpacked, (const void*)bias, (const void*)out, (const void*)out_ds})
    if (!hdn::aligned16(p)) return HDN_E_LIMIT;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (const int rr = hdn::check_fp16_range(x, n_in, s, act_domain)) return rr;
  auto go = [&](auto cfg) {
    using Cf = decltype(cfg);
    return hdn::mc::by_domain(act_domain, [&](auto sd) { return hdn::cvs::launch<Cf, decltype(sd)::value>(x, wpacked, bias, out, out_ds, B, s); });
  };
  if (S == 16 && CI == 64) return go(hdn::cvs::CfgS<16, 64>{});
  if (S == 8 && CI == 128) return go(hdn::cvs::CfgS<8, 128>{});
  if (S == 4 && CI == 256) return go(hdn::cvs::CfgS<4, 256>{});
  return HDN_E_LIMIT;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// hdn_conv3x3s2_f32 — the stride-2 3x3 convolution of a Bottleneck (the first block of layer2 / 3 / 4 of the ResNet-50 trunk), C -> C channels:
//   out[B,S,S,C] = relu(conv3x3/s2/p1(x[B,2S,2S,C], W) + bias[c]),   (S, C) = (16, 128), (8, 256), (4, 512)
// Reference: Bottleneck.forward conv2 + bn2 + relu, homo_estimator/Deep_homography/Oneline_DLTv1/backbone/resnet.py:97-133 (BatchNorm folded by the caller).
//
// The LDS image of the kernel above (a chunk of 32 input channels of the workgroup's (2R + 1) x (2S + 1) input patch as two fp16 pieces, even padded
// columns before odd ones, so that every tap is a constant offset and 16 consecutive lanes read consecutive 16-byte slots) without its producer /
// consumer split: 4 waves stage the chunk together, then each owns a 32 pixel x 32 channel corner of the 64 x 64 output tile and walks the chunk's nine
// taps x two k steps (54 MFMAs per chunk, one barrier pair per chunk; the next chunk's pixels are in flight in registers meanwhile, and two
// workgroups share a CU: 192-202 VGPRs + 32 AGPRs per lane, no scratch, 39-48 KB of LDS each).  Weights go L2 -> registers in fragment order, one kernel row (3 taps) ahead.  The tile leaves through
// the LDS as 16-byte stores.
// K slices: when the output tiles alone give fewer than FILL workgroups (the tracker's B = 1: 8 / 4 / 8 tiles; S = 8 / 4 even at B = 64) grid.z splits K —
// first by chunks, then by kernel row — each slice writes its raw partial tile to `workspace` [z][M][C] and finish_slices (epilogue.hip) adds the slices
// in slice order with the bias and the ReLU: a fixed summation order, no atomics.
// FILL = two workgroups for each of the 256 CUs (what the registers allow to be resident).  Measured with it, rocprofv3 kernel time: docs/KERNELS.md "conv3x3s2".
#ifndef HDN_S2_FILL
#define HDN_S2_FILL 512
#endif

namespace hdn {
namespace cb {
using namespace hdn::mc;

template <int SO_, int C_>
struct CfgB : s2::Image<SO_, 2> {
  using Img = s2::Image<SO_, 2>;
  static constexpr int C = C_, CI = C_;
  static_assert((SO_ == 16 && C == 128) || (SO_ == 8 && C == 256) || (SO_ == 4 && C == 512), "the three stride-2 Bottlenecks of the trunk");
  static constexpr bool PAD_SLOTS = false;
  static constexpr int ASETS = 1;
  static constexpr int NCHUNK = C / (16 * Img::KS), NB = C / Img::BN;
  static constexpr int WTAP = 2 * Img::KS * 2 * 64;                  // 16-byte words of one (channel block, chunk, tap): [n tile][k step][piece][lane]
  static constexpr int RED_BYTES = Img::BM * Img::EPI_STRIDE * 4;
  static constexpr int LDS_BYTES = Img::A_BYTES > RED_BYTES ? Img::A_BYTES : RED_BYTES;
  static_assert(LDS_BYTES <= 64 * 1024, "static LDS");
};

// the K slices of a problem: ZC slices of the chunks x ZT (1 or 3) of the kernel rows
struct Slices {
  int zc, zt;
  int z() const { return zc * zt; }
};
template <class Cf>
static Slices slices_for(long long M) {
  const long long tiles = (M + Cf::BM - 1) / Cf::BM * Cf::NB;
  Slices s{1, 1};
  while (tiles * s.zc < HDN_S2_FILL && s.zc < Cf::NCHUNK) s.zc *= 2;
  if (tiles * s.zc < HDN_S2_FILL) s.zt = 3;
  return s;
}

template <class Cf, bool SD, bool FUSED>
__global__ __launch_bounds__(HDN_BLOCK) void conv3x3s2_kernel(const float* __restrict__ x, const u32x4* __restrict__ wp, const float* __restrict__ bias,
                                                             float* __restrict__ dst, int B, int ZC, int ZT) {
  constexpr int SO = Cf::SO, C = Cf::C, BM = Cf::BM, BN = Cf::BN, KS = Cf::KS;
  __shared__ __attribute__((aligned(16))) unsigned char smem[Cf::LDS_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, g = lane >> 5, wm = wave >> 1, wn = wave & 1;
  const int nb = blockIdx.x;                                  // output-channel block, fastest: neighbours share the input patch in L2
  const long long M = (long long)B * SO * SO;
  const long long m0 = (long long)blockIdx.y * BM;
  const int b0 = (int)(m0 / (SO * SO)), y0 = (int)((m0 % (SO * SO)) / SO);
  const int z = blockIdx.z, zc = z / ZT, zt = z - zc * ZT;
  const int cpz = Cf::NCHUNK / ZC, c0 = zc * cpz;             // this slice's chunks [c0, c0 + cpz) and kernel rows [ky0, ky1)
  const int ky0 = ZT == 3 ? zt : 0, ky1 = ZT == 3 ? zt + 1 : 3;

  s2::Stager<Cf, SD> stager(tid, b0, y0, B);
  const int aoff = Cf::aoff(wm * 32 + li, g);                 // this lane's A row: pixel wm * 32 + li of the tile, tap (0, 0)
  // this wave's weight stream: [channel block][chunk][tap][n tile][k step][piece][lane] x 16 B
  const u32x4* const wbase = wp + (size_t)nb * Cf::NCHUNK * 9 * Cf::WTAP + wn * (Cf::WTAP / 2) + lane;
  u32x4 wnx[3][KS][2];
  auto load_w = [&](int chunk, int ky) {
    const u32x4* p = wbase + ((size_t)chunk * 9 + ky * 3) * Cf::WTAP;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int pc = 0; pc < 2; ++pc) wnx[kx][ks][pc] = p[kx * Cf::WTAP + (ks * 2 + pc) * 64];
  };

  f32x16 hi, lo;
#pragma unroll
  for (int r = 0; r < 16; ++r) hi[r] = lo[r] = 0.f;

  stager.load_a(x, c0);
  load_w(c0, ky0);
  for (int c = 0; c < cpz; ++c) {
    stager.store_a(smem);
    __syncthreads();                                          // chunk c is staged
    if (c + 1 < cpz) stager.load_a(x, c0 + c + 1);
    for (int ky = ky0; ky < ky1; ++ky) {
      u32x4 wv[3][KS][2];
#pragma unroll
      for (int kx = 0; kx < 3; ++kx)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
          for (int pc = 0; pc < 2; ++pc) wv[kx][ks][pc] = wnx[kx][ks][pc];
      if (ky + 1 < ky1) load_w(c0 + c, ky + 1);
      else if (c + 1 < cpz) load_w(c0 + c + 1, ky0);
      const unsigned char* arow = smem + aoff + ky * Cf::PW * 16;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int off = (kx == 0 ? 0 : kx == 1 ? Cf::PWH : 1) * 16;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const u32x4 a0 = *reinterpret_cast<const u32x4*>(arow + off + ks * Cf::KSTEP_BYTES);
          const u32x4 a1 = *reinterpret_cast<const u32x4*>(arow + off + ks * Cf::KSTEP_BYTES + Cf::PIECE_BYTES);
          hi = mfma(a0, wv[kx][ks][0], hi);
          lo = mfma(a0, wv[kx][ks][1], lo);
          lo = mfma(a1, wv[kx][ks][0], lo);
        }
      }
    }
    __syncthreads();                                          // every wave has read chunk c's image
  }

  // the tile -> LDS (over the dead image)
  float* const red = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int r = 0; r < 16; ++r) red[(wm * 32 + d_row(r, g)) * Cf::EPI_STRIDE + wn * 32 + li] = join<SD>(hi[r], lo[r]);
  __syncthreads();
  float* const o = FUSED ? dst : dst + (size_t)z * (size_t)M * C;
  for_tile_items<BM, BN, HDN_BLOCK>(tid, m0, M, [&](int, int px, int c4, long long m) {
    f4 v = *reinterpret_cast<const f4*>(red + px * Cf::EPI_STRIDE + c4 * 4);
    if constexpr (FUSED) v = relu4(v + *reinterpret_cast<const f4*>(bias + nb * BN + c4 * 4));
    *reinterpret_cast<f4*>(o + m * C + nb * BN + c4 * 4) = v;
  });
}

template <class Cf>
static long long workspace_bytes(int B) {
  const long long M = (long long)B * Cf::SO * Cf::SO;
  const int z = slices_for<Cf>(M).z();
  return z > 1 ? (long long)z * M * Cf::C * 4 : 0;
}

template <class Cf, bool SD>
static int launch(const float* x, const void* wp, const float* bias, float* out, float* ws, int B, hipStream_t stream) {   // (ws: checked by the entry)
  const long long M = (long long)B * Cf::SO * Cf::SO, tm = (M + Cf::BM - 1) / Cf::BM;
  const Slices sl = slices_for<Cf>(M);
  if (tm > 65535) return HDN_E_LIMIT;                              // grid.y
  const dim3 grid(Cf::NB, (unsigned)tm, (unsigned)sl.z()), blk(HDN_BLOCK);
  const u32x4* w = static_cast<const u32x4*>(wp);
  if (sl.z() == 1) {
    hipLaunchKernelGGL((conv3x3s2_kernel<Cf, SD, true>), grid, blk, 0, stream, x, w, bias, out, B, 1, 1);
    return launch_status();
  }
  hipLaunchKernelGGL((conv3x3s2_kernel<Cf, SD, false>), grid, blk, 0, stream, x, w, bias, ws, B, sl.zc, sl.zt);
  if (const int rc = launch_status()) return rc;
  return finish_slices(ws, sl.z(), bias, 1, out, M * Cf::C, Cf::C, stream);
}

// f(CfgB<...>{}) for a supported (S, C), HDN_E_LIMIT otherwise
template <class F>
static long long with_cfg(int S, int C, F&& f) {
  if (S == 16 && C == 128) return f(CfgB<16, 128>{});
  if (S == 8 && C == 256) return f(CfgB<8, 256>{});
  if (S == 4 && C == 512) return f(CfgB<4, 512>{});
  return HDN_E_LIMIT;
}

}  // namespace cb
}  // namespace hdn

extern "C" long long hdn_conv3x3s2_workspace_bytes(int B, int S, int C) {
  if (B <= 0) return HDN_E_SHAPE;
  if ((long long)B * S * S * 4 * C > 0x7fffffffLL) return HDN_E_LIMIT;
  return hdn::cb::with_cfg(S, C, [&](auto cfg) { return hdn::cb::workspace_bytes<decltype(cfg)>(B); });
}

// wpacked (hdn_pack_conv3x3s2_f32): [C / 64][C / 32 chunks][9 taps][2 n tiles][2 k steps][2 pieces][k half g][32 n][8] fp16; element e of lane (g, n) =
// piece of w[co = 64 nb + 32 nt + n][ci = 32 chunk + 16 k step + 8 g + e][tap t = 3 ky + kx]
extern "C" int hdn_conv3x3s2_f32(const float* x, const void* wpacked, const float* bias, float* out, float* workspace, long long workspace_bytes, int B,
                                 int S, int C, int act_domain, void* stream) {
  if (!x || !wpacked || !bias || !out) return HDN_E_NULL;
  if (B <= 0 || S <= 0 || C <= 0 || (act_domain != 0 && act_domain != 1)) return HDN_E_SHAPE;
  if (hdn::cb::with_cfg(S, C, [](auto) { return 0; }) != 0) return HDN_E_LIMIT;
  const long long n_out = (long long)B * S * S * C, n_in = 4 * n_out;
  if (n_in > 0x7fffffffLL) return HDN_E_LIMIT;
  if (hdn::bytes_overlap(out, n_out * 4, x, n_in * 4)) return HDN_E_ALIAS;
  for (const void* p : {(const void*)x, wpacked, (const void*)bias, (const void*)out})
    if (!hdn::aligned16(p)) return HDN_E_LIMIT;
  if (const int rc = hdn::check_workspace(workspace, workspace_bytes, hdn_conv3x3s2_workspace_bytes(B, S, C), x, n_in * 4, out, n_out * 4)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (const int rr = hdn::check_fp16_range(x, n_in, s, act_domain)) return rr;
  return (int)hdn::cb::with_cfg(S, C, [&](auto cfg) -> long long {
    using Cf = decltype(cfg);
    return hdn::mc::by_domain(act_domain, [&](auto sd) { return hdn::cb::launch<Cf, decltype(sd)::value>(x, wpacked, bias, out, workspace, B, s); });
  });
}
