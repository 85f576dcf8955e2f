// OpenCV 4.x's INTER_LINEAR warpPerspective walk (modules/imgproc/src/imgwarp.cpp, WarpPerspectiveInvoker), stated once for the float32 warp of
// refine_warp.hip and the 8-bit warp of frame.hip: the 3 x 3 inverse, cvRound, the block geometry and the map from a destination pixel to its
// 1/32-pixel source coordinates and four clamped taps.  The weights and the sums stay with each kernel (float products there, 15-bit integers here).
// Every float64 operation is rounded on its own, in the order written: the including files switch contraction off only after this header, so it
// does so itself, as hdn_common.h does around rn_mul.
#pragma once
#include "hdn_common.h"

#pragma clang fp contract(off)

namespace hdn {

__device__ __forceinline__ void inv3_f64(const double* m, double* o) {
  // adjugate / determinant, as cv::invert does for 3x3 (DECOMP_LU special case)
  const double d = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
  const double id = d != 0.0 ? 1.0 / d : 0.0;
  o[0] = (m[4] * m[8] - m[5] * m[7]) * id;
  o[1] = (m[2] * m[7] - m[1] * m[8]) * id;
  o[2] = (m[1] * m[5] - m[2] * m[4]) * id;
  o[3] = (m[5] * m[6] - m[3] * m[8]) * id;
  o[4] = (m[0] * m[8] - m[2] * m[6]) * id;
  o[5] = (m[2] * m[3] - m[0] * m[5]) * id;
  o[6] = (m[3] * m[7] - m[4] * m[6]) * id;
  o[7] = (m[1] * m[6] - m[0] * m[7]) * id;
  o[8] = (m[0] * m[4] - m[1] * m[3]) * id;
}

__device__ __forceinline__ int cv_round_sat(double v) {
  v = fmax(-2147483648.0, fmin(2147483647.0, v));
  return (int)rint(v);  // round half to even, as cvRound (lrint) does
}

// OpenCV's block walk (BLOCK_SZ 32): destination pixels are walked in bw x bh blocks, which fixes the summation order of x in float64, so bw
// decides bits.  A host launch computes it once; a ragged slot computes its own on the device.
constexpr int RW_BW = 64, RW_BH = 16;  // what it comes to for a 127 x 127 warp
struct CvBlock {
  int bw, bh;
};
__host__ __device__ __forceinline__ CvBlock cv_block(int H, int W) {
  int bh = H < 16 ? H : 16;
  int bw = 1024 / bh < W ? 1024 / bh : W;
  bh = 1024 / bw < H ? 1024 / bw : H;
  return {bw, bh};
}

struct CvPoint {
  int X, Y;            // the source coordinates in 1/32 pixel, rounded half to even and saturated to int32: pixel X >> 5, fraction X & 31
  int x0, x1, y0, y1;  // the taps at X >> 5 and one further, each clamped into the image (BORDER_REPLICATE)
};

// Destination pixel (x, y) of an H x W warp whose INVERSE matrix is mi[9], walked in blocks bw wide: for block column bx + x1
//   X0 = M0*bx + M1*y + M2,  Y0 = M3*bx + M4*y + M5,  W0 = M6*bx + M7*y + M8
//   W = W0 + M6*x1;  W = W ? 32/W : 0;  X = cvRound((X0 + M0*x1)*W),  Y = cvRound((Y0 + M3*x1)*W)
__device__ __forceinline__ CvPoint cv_warp_point(const double* mi, int x, int y, int bw, int H, int W) {
  CvPoint p;
  const int bx = (x / bw) * bw, x1 = x - bx;
  const double X0 = mi[0] * bx + mi[1] * y + mi[2];
  const double Y0 = mi[3] * bx + mi[4] * y + mi[5];
  const double W0 = mi[6] * bx + mi[7] * y + mi[8];
  double Wd = W0 + mi[6] * x1;
  Wd = Wd != 0.0 ? 32.0 / Wd : 0.0;
  p.X = cv_round_sat((X0 + mi[0] * x1) * Wd), p.Y = cv_round_sat((Y0 + mi[3] * x1) * Wd);
  const int sx = p.X >> 5, sy = p.Y >> 5;
  // sx + 1 in 64 bits: a saturated coordinate must not wrap
  p.x0 = min(max(sx, 0), W - 1), p.x1 = (int)min(max((long long)sx + 1, 0LL), (long long)W - 1);
  p.y0 = min(max(sy, 0), H - 1), p.y1 = (int)min(max((long long)sy + 1, 0LL), (long long)H - 1);
  return p;
}

}  // namespace hdn

#pragma clang fp contract(fast)
