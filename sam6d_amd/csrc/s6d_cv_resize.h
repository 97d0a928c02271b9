// cv2.resize(INTER_LINEAR) on CV_8U restated exactly, one output pixel at a time: shared by the per-detection colour crops
// (s6d_pempre.hip pem_crops_kernel) and the template crops of the onboarding (s6d_onboard.hip).
//
// OpenCV 4.x modules/imgproc/src/resize.cpp; oracle/pem_pre.py cv2_resize_linear_u8 is the same statement in numpy: per axis
// scale = 1. / (double(S) / n),  f = (float)((o + 0.5) * scale - 0.5),  s = floor(f),  f -= s;
// x axis: s < 0 -> (0, f = 0), s >= n - 1 -> (n - 1, f = 0); y axis: the two row indices are clipped instead; coefficients
// saturate_cast<short>((1 - f) * 2048), saturate_cast<short>(f * 2048) (round half to even, each on its own);
// t = S[sx] a0 + S[sx + 1] a1 per row (int32), dst = (((b0 (t0 >> 4)) >> 16) + ((b1 (t1 >> 4)) >> 16) + 2) >> 2.
// An exact 2:1 ratio on both axes takes OpenCV's area substitute (four-pixel sum + 2) >> 2, a 1:1 ratio is a copy.
#pragma once
#include "s6d_common.h"

namespace s6d {

__device__ __forceinline__ void cv_linear_tap(int o, int S, long n, bool clamp_index, long &s, int &c0, int &c1) {
#pragma clang fp contract(off)   // the published expressions, operation by operation (no fused multiply-adds)
  const double inv = (double)S / (double)n;
  const double scale = 1.0 / inv;
  float f = (float)(((double)o + 0.5) * scale - 0.5);
  const float fl = floorf(f);
  s = (long)fl;
  f -= fl;
  if (clamp_index) {
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= n - 1) { f = 0.f; s = n - 1; }
  }
  c0 = (int)fminf(fmaxf(rintf((1.f - f) * 2048.f), -32768.f), 32767.f);
  c1 = (int)fminf(fmaxf(rintf(f * 2048.f), -32768.f), 32767.f);
}

// grey level of output pixel (oy, ox) of an h x w crop resized to S x S; px(y, x) -> the crop's uint8 value as an int
template <class Px>
__device__ __forceinline__ int cv_resize_linear_px(Px px, int oy, int ox, long h, long w, int S) {
  if (h == S && w == S) return px((long)oy, (long)ox);
  if (h == 2 * (long)S && w == 2 * (long)S)
    return (px(2L * oy, 2L * ox) + px(2L * oy, 2L * ox + 1) + px(2L * oy + 1, 2L * ox) + px(2L * oy + 1, 2L * ox + 1) + 2) >> 2;
  long sx, sy;
  int a0, a1, b0, b1;
  cv_linear_tap(ox, S, w, true, sx, a0, a1);
  cv_linear_tap(oy, S, h, false, sy, b0, b1);
  const long ya = min(max(sy, 0L), h - 1), yb = min(max(sy + 1, 0L), h - 1), xb = min(sx + 1, w - 1);
  const int t0 = px(ya, sx) * a0 + px(ya, xb) * a1;
  const int t1 = px(yb, sx) * a0 + px(yb, xb) * a1;
  const int g = (((b0 * (t0 >> 4)) >> 16) + ((b1 * (t1 >> 4)) >> 16) + 2) >> 2;
  return min(max(g, 0), 255);
}

}  // namespace s6d
