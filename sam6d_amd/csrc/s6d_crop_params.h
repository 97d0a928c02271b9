// Geometry of CropResizePad.__call__ (Instance_Segmentation_Model/utils/bbox_utils.py:98-126) with ATen's nearest index rule, and the
// reference's square crop box: shared by the proposal crops (s6d_crop.hip), the template crops of the onboarding (s6d_onboard.hip)
// and the mask boxes of both (s6d_compact.h).  The host side (sam6d_amd/ism/dinov2.py crop_params) fills one record per crop.
#pragma once
#include "s6d_common.h"

namespace s6d {

struct CropParams {     // 12 x 4 bytes; all sizes in pixels
  int x1, y1;           // crop origin in the frame
  int h, w;             // crop size (box[3]-box[1], box[2]-box[0]: the max corner is EXCLUDED, as in the reference)
  int h1, w1;           // size after the first resize: floor(h * s1), floor(w * s1)
  int top, left;        // zero padding in front of the resized crop
  int S2;               // side of the padded square
  float inv1, inv2;     // float(1 / s1), float(1 / s2): ATen's compute_scales_value<float>
  int pad_;
};

__device__ __forceinline__ int nearest_src(int dst, int in, float inv) {
  return min((int)floorf((float)dst * inv), in - 1);
}

// Output pixel o of the S x S crop of record c -> its source pixel (sy, sx) in the H x W frame: the second resize (padded square -> S),
// the padding, the first resize (crop -> h1 x w1).  false = padding; a source outside the frame (never one of a record of crop_params)
// is padding too, so no record makes a kernel read outside its maps.
__device__ __forceinline__ bool crop_src(const CropParams &c, int o, int S, int H, int W, int &sy, int &sx) {
  const int oy = o / S, ox = o - oy * S;
  const int py = nearest_src(oy, c.S2, c.inv2), px = nearest_src(ox, c.S2, c.inv2);
  const int iy = py - c.top, ix = px - c.left;
  if (iy < 0 || iy >= c.h1 || ix < 0 || ix >= c.w1) return false;
  sy = c.y1 + nearest_src(iy, c.h, c.inv1);
  sx = c.x1 + nearest_src(ix, c.w, c.inv1);
  return sy >= 0 && sy < H && sx >= 0 && sx < W;
}

// pixel o of the three S x S colour planes of one crop
__device__ __forceinline__ void store_rgb_planes(float *crop, int o, int S, float r, float g, float b) {
  const size_t plane = (size_t)S * S;
  crop[o] = r;
  crop[plane + o] = g;
  crop[2 * plane + o] = b;
}

// The reference's square crop box, get_bbox (Pose_Estimation_Model/utils/data_utils.py:126-160), from the extent of a pixel set:
// rows [rmin, rmax) and columns [cmin, cmax), the whole frame where the caller finds no set.  The longer side, at most min(H, W),
// centred on the extent and pushed back inside the frame.  box = [rmin, rmax, cmin, cmax].  Shared by the per-frame mask boxes
// (s6d_pempre.hip) and the template boxes of the onboarding (s6d_onboard.hip); which pixels form the set is the caller's rule.
__device__ __forceinline__ void square_box(long rmin, long rmax, long cmin, long cmax, int H, int W, long *box) {
  const long rb = rmax - rmin, cb = cmax - cmin, lim = H < W ? H : W;
  long side = rb > cb ? rb : cb;
  side = side < lim ? side : lim;
  const long cy = (rmin + rmax) / 2, cx = (cmin + cmax) / 2, half = side / 2;
  rmin = cy - half;
  rmax = cy + half;
  cmin = cx - half;
  cmax = cx + half;
  if (rmin < 0) {
    rmax -= rmin;
    rmin = 0;
  }
  if (cmin < 0) {
    cmax -= cmin;
    cmin = 0;
  }
  if (rmax > H) {
    rmin -= rmax - H;
    rmax = H;
  }
  if (cmax > W) {
    cmin -= cmax - W;
    cmax = W;
  }
  box[0] = rmin;
  box[1] = rmax;
  box[2] = cmin;
  box[3] = cmax;
}

static_assert(sizeof(CropParams) == 48, "CropParams is the 12-int record of include/sam6d_hip.h");

}  // namespace s6d
