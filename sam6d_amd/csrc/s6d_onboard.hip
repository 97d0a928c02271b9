// Kernels of the object onboarding: from the rendered template views of an object (rgb_i.png, mask_i.png, xyz_i.npy) to the
// inputs of the two onboarding passes (host side: sam6d_amd/onboarding.py).  The per-frame twins are s6d_pempre.hip and s6d_crop.hip;
// here every view is an image of its own with its own xyz map and "set" means == 255.  What the twins have in common is written once
// (s6d_compact.h, s6d_crop_params.h, s6d_cv_resize.h) with its guards: a box or a crop record that reaches outside the view is
// skipped or written as padding, never read.
//
//   template_boxes   one pass over every view's mask for the two boxes the reference takes from it: the square get_bbox crop of
//                    the pixels == 255 (Pose_Estimation_Model/run_inference_custom.py:124-127, utils/data_utils.py:126-160) and
//                    PIL's getbbox of the pixels != 0 (Instance_Segmentation_Model/run_inference_custom.py:131-132).
//   template_points  "mask -> choose -> xyz" of _get_template (:128, :137, :143): the pixels == 255 of the square crop in row-major
//                    crop order with their model points, xyz / 1000 as the float32 division numpy performs (:123).
//   pem_crops        the colour crop of _get_template (:130-135): pem_crops_kernel<ViewCrops> of s6d_cv_resize.h.
//   ism_crops        the template block of the ISM (Instance_Segmentation_Model/run_inference_custom.py:134-151, provider/bop.py:
//                    60-83): fl32(u8 / 255) * fl32(mask / 255), CropResizePad, and (BOP flow) Normalize AFTER the crop.
// The sampler of :138-141 is s6d_pem_sample_indices_f32 (s6d_pempre.hip), which serves n_sample = 5000.
#include "s6d_common.h"
#include "s6d_compact.h"
#include "s6d_crop_params.h"
#include "s6d_cv_resize.h"

namespace s6d {

#pragma clang fp contract(off)   // the reference's float32 expressions, operation by operation (no fused multiply-adds)

// mask (T,H,W) u8 -> cnt (T) i64 pixels == 255, box (T,4) i64 [y1,y2,x1,x2] = get_bbox of them (of the whole view when there is none),
// tight (T,4) i64 [x1,y1,x2,y2] = PIL getbbox of the pixels != 0 (zeros when there is none).  One workgroup per view.
__global__ __launch_bounds__(kCmpThreads) void template_boxes_kernel(const unsigned char *__restrict__ mask, int H, int W,
                                                                    long *__restrict__ cnt_out, long *__restrict__ box,
                                                                    long *__restrict__ tight) {
  const int t = blockIdx.x, tid = threadIdx.x;
  const unsigned char *mp = mask + (size_t)t * H * W;
  int cnt = 0, b[8];                                                 // extents of the pixels == 255, then of the pixels != 0
  extent_init(b, H, W);
  extent_init(b + 4, H, W);
  for (int i = tid; i < H * W; i += kCmpThreads) {
    const unsigned char v = mp[i];
    if (v != 0) {
      const int y = i / W, x = i - y * W;
      extent_add(b + 4, y, x);
      if (v == 255) {
        ++cnt;
        extent_add(b, y, x);
      }
    }
  }
  const long c = block_extents<2>(cnt, b);
  if (tid == 0) {
    cnt_out[t] = c;
    extent_box(c > 0, b, H, W, box + t * 4);
    const bool any = b[5] >= 0;
    tight[t * 4 + 0] = any ? -b[6] : 0;
    tight[t * 4 + 1] = any ? -b[4] : 0;
    tight[t * 4 + 2] = any ? b[7] + 1 : 0;
    tight[t * 4 + 3] = any ? b[5] + 1 : 0;
  }
}

// mask (T,H,W) u8, xyz (T,H,W,3) f32 millimetres, box (T,4) i64 [y1,y2,x1,x2]
// -> choose (T,cap) i32 crop-flat indices, pts (T,cap,3) f32 metres, n (T) i64.  One workgroup per view.
__global__ __launch_bounds__(kCmpThreads) void template_points_kernel(const unsigned char *__restrict__ mask,
                                                                     const float *__restrict__ xyz,
                                                                     const long *__restrict__ box, int H, int W, long cap,
                                                                     int *__restrict__ choose, float *__restrict__ pts,
                                                                     long *__restrict__ n_out) {
  const int t = blockIdx.x;
  const unsigned char *mp = mask + (size_t)t * H * W;
  const float *xp = xyz + (size_t)t * H * W * 3;
  compact_crop(
      box + t * 4, true, H, W, cap, n_out + t, [&](int pix) { return mp[pix] == 255; },
      [&](long pos, int j, int y, int x) {
        const float *q = xp + ((size_t)y * W + x) * 3;
        choose[(size_t)t * cap + pos] = j;
        float *d = pts + ((size_t)t * cap + pos) * 3;
        d[0] = q[0] / 1000.0f;
        d[1] = q[1] / 1000.0f;
        d[2] = q[2] / 1000.0f;
      });
}

// images (T,H,W,3) u8, mask (T,H,W) u8, params (T) records -> out_rgb (T,3,S,S) f32 and / or out_mask (T,S,S) f32
__global__ __launch_bounds__(256) void template_ism_crops_kernel(const unsigned char *__restrict__ images,
                                                                 const unsigned char *__restrict__ mask,
                                                                 const CropParams *__restrict__ params, int H, int W, int S,
                                                                 int normalize, float m0, float m1, float m2, float s0,
                                                                 float s1, float s2, float *__restrict__ out_rgb,
                                                                 float *__restrict__ out_mask) {
  const int t = blockIdx.y;
  const int o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= S * S) return;
  int sy, sx;
  float r = 0.f, g = 0.f, b = 0.f, mk = 0.f;
  if (crop_src(params[t], o, S, H, W, sy, sx)) {
    const size_t pix = ((size_t)t * H + sy) * W + sx;
    mk = (float)mask[pix] / 255.0f;
    if (out_rgb) {
      const unsigned char *q = images + pix * 3;
      r = ((float)q[0] / 255.0f) * mk;
      g = ((float)q[1] / 255.0f) * mk;
      b = ((float)q[2] / 255.0f) * mk;
    }
  }
  if (out_rgb) {
    if (normalize) {                                                   // rgb_transform after the crop: the padding too
      r = (r - m0) / s0;
      g = (g - m1) / s1;
      b = (b - m2) / s2;
    }
    store_rgb_planes(out_rgb + (size_t)t * 3 * S * S, o, S, r, g, b);
  }
  if (out_mask) out_mask[(size_t)t * S * S + o] = mk;
}

}  // namespace s6d

using namespace s6d;

extern "C" int s6d_template_boxes_u8(const unsigned char *mask, int T, int H, int W, int64_t *cnt, int64_t *box, int64_t *tight,
                                     void *stream) {
  if (T < 0 || H <= 0 || W <= 0 || (long)H * W > 0x7fffffffL) return S6D_EINVAL;
  if (T == 0) return S6D_OK;
  if (!mask || !cnt || !box || !tight) return S6D_EINVAL;
  hipLaunchKernelGGL(template_boxes_kernel, dim3((unsigned)T), dim3(kCmpThreads), 0, as_stream(stream), mask, H, W, (long *)cnt,
                     (long *)box, (long *)tight);
  return launch_status();
}

extern "C" int s6d_template_points_f32(const unsigned char *mask, const float *xyz_mm, const int64_t *box, int T, int H, int W,
                                       long cap, int32_t *choose, float *pts, int64_t *n, void *stream) {
  if (T < 0 || H <= 0 || W <= 0 || (long)H * W > 0x7fffffffL || cap <= 0) return S6D_EINVAL;
  if (T == 0) return S6D_OK;
  if (!mask || !xyz_mm || !box || !choose || !pts || !n) return S6D_EINVAL;
  hipLaunchKernelGGL(template_points_kernel, dim3((unsigned)T), dim3(kCmpThreads), 0, as_stream(stream), mask, xyz_mm,
                     (const long *)box, H, W, cap, choose, pts, (long *)n);
  return launch_status();
}

extern "C" int s6d_template_pem_crops_f32(const unsigned char *images, const unsigned char *mask, const int64_t *box, int T, int H,
                                          int W, int S, int use_mask, const float *mean3_host, const float *std3_host, float *out,
                                          void *stream) {
  if (T < 0 || H <= 0 || W <= 0 || S <= 0 || (long)H * W > 0x7fffffffL) return S6D_EINVAL;
  if (T == 0) return S6D_OK;
  if (!images || !mask || !box || !mean3_host || !std3_host || !out) return S6D_EINVAL;
  const size_t total = (size_t)T * 3 * S * S;
  size_t g = (total + 255) / 256;
  if (g > 16384) g = 16384;
  const ViewCrops src{images, mask};
  hipLaunchKernelGGL(pem_crops_kernel<ViewCrops>, dim3((unsigned)g), dim3(256), 0, as_stream(stream), src, (const long *)box, T, H, W,
                     S, use_mask, mean3_host[0], mean3_host[1], mean3_host[2], std3_host[0], std3_host[1], std3_host[2], out);
  return launch_status();
}

extern "C" int s6d_template_ism_crops_f32(const unsigned char *images, const unsigned char *mask, const void *params, int T, int H,
                                          int W, int S, int normalize, const float *mean3_host, const float *std3_host,
                                          float *out_rgb, float *out_mask, void *stream) {
  if (T < 0 || T > 65535 || H <= 0 || W <= 0 || S <= 0 || S > 4096 || (long)H * W > 0x7fffffffL) return S6D_EINVAL;
  if (T == 0) return S6D_OK;
  if (!mask || !params || (!out_rgb && !out_mask) || (out_rgb && (!images || (normalize && (!mean3_host || !std3_host)))))
    return S6D_EINVAL;
  const float one[3] = {1.f, 1.f, 1.f}, zero[3] = {0.f, 0.f, 0.f};
  const bool nrm = out_rgb && normalize;
  const float *m = nrm ? mean3_host : zero, *s = nrm ? std3_host : one;
  const dim3 grid((unsigned)((S * S + 255) / 256), (unsigned)T);
  hipLaunchKernelGGL(template_ism_crops_kernel, grid, dim3(256), 0, as_stream(stream), images, mask, (const CropParams *)params,
                     H, W, S, nrm ? 1 : 0, m[0], m[1], m[2], s[0], s[1], s[2], out_rgb, out_mask);
  return launch_status();
}
