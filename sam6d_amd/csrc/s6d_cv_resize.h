// cv2.resize(INTER_LINEAR) on CV_8U restated exactly, one output pixel at a time, and the colour crop kernel built on it: one
// template for the per-detection crops (s6d_pempre.hip, FrameCrops) and the template crops of the onboarding (s6d_onboard.hip,
// ViewCrops).
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

// Where output item k of pem_crops_kernel comes from: its row of the mask planes and of the boxes, its image, and which mask values
// count as set.  FrameCrops: detection kept[k] (unchecked: the C ABI does not pass P) of the one frame, set = non-zero.
struct FrameCrops {
  const unsigned char *image, *mask;
  const long *kept;
  __device__ long row(int k) const { return kept[k]; }
  __device__ const unsigned char *pixels(long, size_t) const { return image; }
  __device__ static bool set(unsigned char v) { return v != 0; }
};

// ViewCrops: template view k with an image of its own, set = 255.
struct ViewCrops {
  const unsigned char *image, *mask;
  __device__ long row(int k) const { return k; }
  __device__ const unsigned char *pixels(long p, size_t hw) const { return image + (size_t)p * hw * 3; }
  __device__ static bool set(unsigned char v) { return v == 255; }
};

// Colour crop of every item, masked (use_mask), resized to S x S and normalised (Pose_Estimation_Model/run_inference_custom.py:
// 229-236 per detection, :130-135 per template view: uint8 crop * uint8 mask, cv2.resize(INTER_LINEAR), ToTensor + Normalize).
// images u8 RGB (H,W,3 each), mask planes (H,W) u8, box rows i64 [y1,y2,x1,x2] -> out (M,3,S,S) f32, channel c = image channel 2 - c.
// A box that does not lie inside the view (never one of the boxes kernels') gives (0 - mean) / std: no read outside the maps.
template <class Src>
__global__ void pem_crops_kernel(Src src, const long *__restrict__ box, int M, int H, int W, int S, int use_mask, float mean0,
                                 float mean1, float mean2, float std0, float std1, float std2, float *__restrict__ out) {
#pragma clang fp contract(off)   // the reference's float32 expressions, operation by operation (no fused multiply-adds)
  const size_t total = (size_t)M * 3 * S * S;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int ox = (int)(i % S), oy = (int)((i / S) % S), c = (int)((i / ((size_t)S * S)) % 3), k = (int)(i / ((size_t)3 * S * S));
    const long p = src.row(k);
    const long y1 = box[p * 4 + 0], y2 = box[p * 4 + 1], x1 = box[p * 4 + 2], x2 = box[p * 4 + 3];
    const long h = y2 - y1, w = x2 - x1;
    const float mean = c == 0 ? mean0 : (c == 1 ? mean1 : mean2), sd = c == 0 ? std0 : (c == 1 ? std1 : std2);
    if (y1 < 0 || h <= 0 || y2 > H || x1 < 0 || w <= 0 || x2 > W) {
      out[i] = (0.f - mean) / sd;
      continue;
    }
    const int ch = 2 - c;
    const unsigned char *ip = src.pixels(p, (size_t)H * W), *mp = src.mask + (size_t)p * H * W;
    auto px = [&](long yy, long xx) -> int {                           // uint8 crop * uint8 mask of the reference
      const long y = y1 + yy, x = x1 + xx;
      const int v = (int)ip[(y * W + x) * 3 + ch];
      return use_mask ? (Src::set(mp[y * W + x]) ? v : 0) : v;
    };
    const int g = cv_resize_linear_px(px, oy, ox, h, w, S);
    out[i] = ((float)g / 255.f - mean) / sd;
  }
}

}  // namespace s6d
