// What the trunk's 3x3 matrix-core convolutions share beyond mfma_split.h (conv3x3.hip: conv3x3_kernel and conv3x3_v2_kernel; conv3x3s2.hip): the LDS
// activation image of the stride-1 / round-4 kernels (HaloImage) with the lane -> pixel order its bank mapping relies on, the split-and-store of one
// staged item, the accumulator tile -> LDS step and the walk of an LDS tile to 16-byte NHWC items.
#pragma once
#include "hdn_common.h"
#include "mfma_split.h"

namespace hdn {
namespace mc {

// Row i (0..31) of an MFMA tile -> pixel of the tile's 32-pixel block, (image, y, x) order.  Stride-1 tiles with rows shorter than
// 32 pixels hand the two 16-lane access groups of a fragment read pixel sets that are 16 distinct columns of the bank row:
// group = which of the two, k = rank inside it; S = 16: group = row; S = 8: rows (0, 2) | (1, 3); S = 4: even | odd rows of two images.
template <int S>
__host__ __device__ constexpr __forceinline__ int mrow_to_pixel_s1(int i) {   // stride-1 tiles of side S
  if constexpr (S >= 32) {
    return i;
  } else {
    const int q = i >> 2, grp = (0x96 >> q) & 1, k = ((q >> 1) << 2) | (i & 3);
    if constexpr (S == 16) return grp * 16 + k;
    else if constexpr (S == 8) return (2 * (k >> 3) + grp) * 8 + (k & 7);
    else return (k >> 3) * 16 + (2 * ((k >> 2) & 1) + grp) * 4 + (k & 3);
  }
}
template <class Cf>
__host__ __device__ constexpr __forceinline__ int mrow_to_pixel(int i) {
  if constexpr (Cf::STRIDE != 1) return i;
  else return mrow_to_pixel_s1<Cf::S>(i);
}

// The LDS activation image: one K chunk of 16 KS input channels of the input patch, with its one-pixel halo (zeros outside the image), of a tile of BM
// output pixels (consecutive in (b, y, x) order: whole rows of one image, or whole images) of side S at stride STRIDE, as
// [piece][k step][k half][pixel slot] x 16 B: an MFMA A fragment (lane = (pixel row i, k half g), 8 fp16) is one ds_read_b128 and a tap is a
// constant address offset.
template <int S_, int STRIDE_, int BM_, int KS_>
struct HaloImage {
  static constexpr int S = S_, STRIDE = STRIDE_, SI = S * STRIDE, BM = BM_, KS = KS_;
  static_assert(STRIDE == 1 || STRIDE == 2, "stride");
  static_assert((BM % S == 0) && ((S * S) % BM == 0 || BM % (S * S) == 0), "a tile is whole rows of one image, or whole images");
  static constexpr int IMGS = BM > S * S ? BM / (S * S) : 1;      // images per tile
  static constexpr int R = BM / (S * IMGS);                      // output rows per image in the tile
  static constexpr int PWV = SI + 2, PH = STRIDE == 1 ? R + 2 : 2 * R + 1;  // halo'ed input patch
  // Pitches of the LDS image.  A ds_read_b128 is served in groups of 16 lanes ({0-3,12-15,20-27}, {4-11,16-19,28-31} of a half
  // wave), which must fall on 16 different 16-byte columns of the 256-byte bank row.  With image rows shorter than 16 pixels that
  // takes a row pitch of 12 pixels at S = 8 and an image pitch of 40 at S = 4, together with the lane -> pixel order of
  // mrow_to_pixel() above (40 % of the LDS cycles of those stages were bank conflicts before).
  static constexpr int PW = (STRIDE == 1 && S == 8) ? 12 : PWV;
  static constexpr int IPITCH = PH * PW + ((STRIDE == 1 && S == 4) ? 4 : 0);
  // ... and the producers' ds_write_b128 (8 consecutive lanes = 8 / (2 KS) pixels x the 2 KS (k step, k half) sub-images of a pixel, one
  // 128-byte bank row) needs the sub-images 128 / (2 KS) bytes apart modulo 128: LP = 8 / (2 KS) modulo 8.
  static constexpr int LPV = IMGS * IPITCH;                      // LDS pixels that exist
  static constexpr int LP = LPV + ((8 / (2 * KS) - LPV % 8) + 8) % 8;
  static constexpr int NP = 2;                                   // fp16 pieces per value
  static constexpr int KG_BYTES = LP * 16, KSTEP_BYTES = 2 * KG_BYTES, PIECE_BYTES = KS * KSTEP_BYTES, A_BYTES = NP * PIECE_BYTES;
  static constexpr int AITEMS = LP * 2 * KS, AITER = cdiv(AITEMS, HDN_BLOCK);   // (pixel slot, k step, k half) items of 8 channels = 32 bytes of input

  // byte offset in an image of tile pixel p (0 .. BM - 1), k half g, at the tap `tap` padded rows and columns from the top-left one (1: the centre)
  static __device__ __forceinline__ int aoff(int p, int g, int tap) {
    const int img = p / (R * S), yy = (p / S) % R, xx = p % S;
    return g * KG_BYTES + (img * IPITCH + (STRIDE * yy + tap) * PW + (STRIDE * xx + tap)) * 16;
  }
  // ... of staging item (pixel slot px, sub = k step * 2 + k half)
  static __device__ __forceinline__ int item_off(int px, int sub) { return sub * KG_BYTES + px * 16; }
  // Pixel slot px of the image of the tile that starts at output row y0 of image b0 (of B): ok = it is an input pixel (not halo outside the image, not
  // a pad slot, not past the batch), pix = which, (b * SI + y) * SI + x (meaningful only then); ry = the slot's row in the patch.
  struct Source {
    bool ok;
    int ry;
    size_t pix;
  };
  static __device__ __forceinline__ Source source(int px, int b0, int y0, int B) {
    const int img = px / IPITCH, ry = (px % IPITCH) / PW, rx = px % IPITCH % PW;
    const int b = b0 + img, y = STRIDE * y0 + ry - 1, xx = rx - 1;
    return {img < IMGS && b < B && ry < PH && y >= 0 && y < SI && xx >= 0 && xx < SI, ry, ((size_t)b * SI + y) * SI + xx};
  }
};

constexpr int epi_stride(int BN) { return BN + 4; }   // floats per pixel row of an output tile in LDS (pad: bank spread of the two half waves)

// eight consecutive fp32 values (u, then v) of a staging item -> their two pieces at `dst` of the image's two piece planes
template <class Cf, bool SD>
__device__ __forceinline__ void split_store(const f4& u, const f4& v, unsigned char* dst) {
  u32x4 p0, p1;
  split8<SD>(u, v, p0, p1);
  *reinterpret_cast<u32x4*>(dst) = p0;
  *reinterpret_cast<u32x4*>(dst + Cf::PIECE_BYTES) = p1;
}

// A wave's MT x NT accumulator tiles (hi, lo) -> the fp32 output tile in LDS, `base` = the wave's first pixel row, its first column + (lane & 31);
// PIX = the lane -> pixel order of a 32-row MFMA tile, g = lane >> 5.  The pixel of accumulator row d_row(r, g) is a compile-time constant for
// each of the two half waves: one multiply-add per store instead of the mapping's dozen integer operations (round 5).
template <int (*PIX)(int), bool SD, int EPI_STRIDE, int MT, int NT>
__device__ __forceinline__ void acc_to_lds(const f32x16 (&hi)[MT][NT], const f32x16 (&lo)[MT][NT], float* base, int g) {
  static_for<MT>([&](auto MTc) {
    static_for<16>([&](auto Rc) {
      constexpr int mt = decltype(MTc)::value, r = decltype(Rc)::value, i0 = d_row(r);
      constexpr int row0 = mt * 32 + PIX(i0), row1 = mt * 32 + PIX(i0 + 4);
      float* const q = base + (row0 + g * (row1 - row0)) * EPI_STRIDE;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) q[nt * 32] = join<SD>(hi[mt][nt][r], lo[mt][nt][r]);
    });
  });
}

// f(q, px, c4, m) for the 16-byte items of a BM x BN tile (pixel rows m0 + px < M, channels 4 c4 ..) dealt to THREADS threads, item tid + q THREADS to
// thread tid < THREADS: a pixel's BN channels (contiguous in NHWC) are BN / 4 consecutive lanes.  CLAMP: every thread's every q, past the tile and past M too,
// with m clamped to the last pixel - an unconditional prefetch (the residual) that stays in registers.
constexpr int tile_iters(int BM, int BN, int THREADS) { return cdiv(BM * (BN / 4), THREADS); }   // items per thread
template <int BM, int BN, int THREADS, bool CLAMP = false, class F>
__device__ __forceinline__ void for_tile_items(int tid, long long m0, long long M, F&& f) {
  constexpr int N4 = BN / 4, TOT4 = BM * N4;
#pragma unroll
  for (int q = 0; q < tile_iters(BM, BN, THREADS); ++q) {
    const int idx = tid + q * THREADS, px = idx / N4, c4 = idx % N4;
    const long long m = CLAMP ? min(m0 + px, M - 1) : m0 + px;
    if (CLAMP || ((TOT4 % THREADS == 0 || idx < TOT4) && m < M)) f(q, px, c4, m);
  }
}

}  // namespace mc
}  // namespace hdn
