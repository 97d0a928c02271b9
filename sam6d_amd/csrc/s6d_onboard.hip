// Kernels of the object onboarding: from the rendered template views of an object (rgb_i.png, mask_i.png, xyz_i.npy) to the
// inputs of the two onboarding passes (host side: sam6d_amd/onboarding.py).  The per-frame twin is s6d_pempre.hip; here every
// view is an image of its own with its own xyz map.
//
//   template_boxes   one pass over every view's mask for the two boxes the reference takes from it: the square get_bbox crop of
//                    the pixels == 255 (Pose_Estimation_Model/run_inference_custom.py:124-127, utils/data_utils.py:126-160) and
//                    PIL's getbbox of the pixels != 0 (Instance_Segmentation_Model/run_inference_custom.py:131-132).
//   template_points  "mask -> choose -> xyz" of _get_template (:128, :137, :143): the pixels == 255 of the square crop in row-major
//                    crop order with their model points, xyz / 1000 as the float32 division numpy performs (:123).
//   pem_crops        the colour crop of _get_template (:130-135): s6d_pem_crops_f32's arithmetic with one image per crop.
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
  constexpr int kWaves = kCmpThreads / 64;
  __shared__ int s_cnt[kWaves], s_b[8][kWaves];
  const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned char *mp = mask + (size_t)t * H * W;
  // [0..3]: y0, y1, x0, x1 of the pixels == 255; [4..7]: of the pixels != 0 (minima kept negated: one max-reduction for all)
  int cnt = 0, b[8] = {-H, -1, -W, -1, -H, -1, -W, -1};
  for (int i = tid; i < H * W; i += kCmpThreads) {
    const unsigned char v = mp[i];
    if (v != 0) {
      const int y = i / W, x = i - y * W;
      b[4] = max(b[4], -y);
      b[5] = max(b[5], y);
      b[6] = max(b[6], -x);
      b[7] = max(b[7], x);
      if (v == 255) {
        ++cnt;
        b[0] = max(b[0], -y);
        b[1] = max(b[1], y);
        b[2] = max(b[2], -x);
        b[3] = max(b[3], x);
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cnt += __shfl_xor(cnt, o);
#pragma unroll
    for (int k = 0; k < 8; ++k) b[k] = max(b[k], __shfl_xor(b[k], o));
  }
  if (lane == 0) {
    s_cnt[wave] = cnt;
#pragma unroll
    for (int k = 0; k < 8; ++k) s_b[k][wave] = b[k];
  }
  __syncthreads();
  if (tid == 0) {
    long c = 0;
    int r[8] = {-H, -1, -W, -1, -H, -1, -W, -1};
    for (int w = 0; w < kWaves; ++w) {
      c += s_cnt[w];
      for (int k = 0; k < 8; ++k) r[k] = max(r[k], s_b[k][w]);
    }
    const bool ok = c > 0;
    cnt_out[t] = c;
    square_box(ok ? -r[0] : 0, ok ? r[1] + 1 : H, ok ? -r[2] : 0, ok ? r[3] + 1 : W, H, W, box + t * 4);
    const bool any = r[5] >= 0;
    tight[t * 4 + 0] = any ? -r[6] : 0;
    tight[t * 4 + 1] = any ? -r[4] : 0;
    tight[t * 4 + 2] = any ? r[7] + 1 : 0;
    tight[t * 4 + 3] = any ? r[5] + 1 : 0;
  }
}

// mask (T,H,W) u8, xyz (T,H,W,3) f32 millimetres, box (T,4) i64 [y1,y2,x1,x2] inside the view
// -> choose (T,cap) i32 crop-flat indices, pts (T,cap,3) f32 metres, n (T) i64.  One workgroup per view.
__global__ __launch_bounds__(kCmpThreads) void template_points_kernel(const unsigned char *__restrict__ mask,
                                                                     const float *__restrict__ xyz,
                                                                     const long *__restrict__ box, int H, int W, long cap,
                                                                     int *__restrict__ choose, float *__restrict__ pts,
                                                                     long *__restrict__ n_out) {
  __shared__ unsigned wave_tot[kCmpThreads / 64];
  __shared__ long base;
  const int t = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) base = 0;
  __syncthreads();
  const long y1 = box[t * 4 + 0], y2 = box[t * 4 + 1], x1 = box[t * 4 + 2], x2 = box[t * 4 + 3];
  // a box that does not lie inside the view (not one of template_boxes') is skipped whole: no read outside the maps
  const bool inside = y1 >= 0 && y1 <= y2 && y2 <= H && x1 >= 0 && x1 <= x2 && x2 <= W && (y2 - y1) * (x2 - x1) <= cap;
  if (inside) {
    const int bw = (int)(x2 - x1), area = (int)(y2 - y1) * bw;    // a crop is at most H * W < 2^31 pixels: 32-bit index arithmetic
    const unsigned char *mp = mask + (size_t)t * H * W;
    const float *xp = xyz + (size_t)t * H * W * 3;
    for (int c0 = 0; c0 < area; c0 += kCmpThreads) {
      const int j = c0 + tid;
      bool keep = false;
      size_t pix = 0;
      if (j < area) {
        const int r = j / bw;
        pix = (size_t)((int)y1 + r) * W + ((int)x1 + (j - r * bw));
        keep = mp[pix] == 255;
      }
      const long pos = block_rank(keep, &base, wave_tot);
      if (keep) {
        choose[(size_t)t * cap + pos] = j;
        float *d = pts + ((size_t)t * cap + pos) * 3;
        d[0] = xp[pix * 3 + 0] / 1000.0f;
        d[1] = xp[pix * 3 + 1] / 1000.0f;
        d[2] = xp[pix * 3 + 2] / 1000.0f;
      }
    }
  }
  __syncthreads();
  if (tid == 0) n_out[t] = base;
}

// images (T,H,W,3) u8 RGB, mask (T,H,W) u8, box (T,4) i64 -> out (T,3,S,S) f32, channel c = image channel 2 - c
__global__ void template_pem_crops_kernel(const unsigned char *__restrict__ images, const unsigned char *__restrict__ mask,
                                          const long *__restrict__ box, int T, int H, int W, int S, int use_mask, float mean0,
                                          float mean1, float mean2, float std0, float std1, float std2,
                                          float *__restrict__ out) {
  const size_t total = (size_t)T * 3 * S * S;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int ox = (int)(i % S), oy = (int)((i / S) % S), c = (int)((i / ((size_t)S * S)) % 3), t = (int)(i / ((size_t)3 * S * S));
    const long y1 = box[t * 4 + 0], y2 = box[t * 4 + 1], x1 = box[t * 4 + 2], x2 = box[t * 4 + 3];
    const long h = y2 - y1, w = x2 - x1;
    const float mean = c == 0 ? mean0 : (c == 1 ? mean1 : mean2), sd = c == 0 ? std0 : (c == 1 ? std1 : std2);
    if (y1 < 0 || h <= 0 || y2 > H || x1 < 0 || w <= 0 || x2 > W) {      // not a box of template_boxes: no read outside the view
      out[i] = (0.f - mean) / sd;
      continue;
    }
    const int ch = 2 - c;
    const unsigned char *ip = images + (size_t)t * H * W * 3, *mp = mask + (size_t)t * H * W;
    auto px = [&](long yy, long xx) -> int {                           // uint8 crop * (mask == 255) of the reference
      const long y = y1 + yy, x = x1 + xx;
      const int v = (int)ip[(y * W + x) * 3 + ch];
      return use_mask ? (mp[y * W + x] == 255 ? v : 0) : v;
    };
    const int g = cv_resize_linear_px(px, oy, ox, h, w, S);
    out[i] = ((float)g / 255.f - mean) / sd;
  }
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
  const CropParams c = params[t];
  const int oy = o / S, ox = o - oy * S;
  const int py = nearest_src(oy, c.S2, c.inv2), px = nearest_src(ox, c.S2, c.inv2);      // second resize: padded square -> S
  const int iy = py - c.top, ix = px - c.left;                                           // padding
  float r = 0.f, g = 0.f, b = 0.f, mk = 0.f;
  if (iy >= 0 && iy < c.h1 && ix >= 0 && ix < c.w1) {
    const int sy = c.y1 + nearest_src(iy, c.h, c.inv1), sx = c.x1 + nearest_src(ix, c.w, c.inv1);      // first resize
    if (sy >= 0 && sy < H && sx >= 0 && sx < W) {                      // (a record of crop_params always is)
      const size_t pix = ((size_t)t * H + sy) * W + sx;
      mk = (float)mask[pix] / 255.0f;
      if (out_rgb) {
        const unsigned char *q = images + pix * 3;
        r = ((float)q[0] / 255.0f) * mk;
        g = ((float)q[1] / 255.0f) * mk;
        b = ((float)q[2] / 255.0f) * mk;
      }
    }
  }
  const size_t plane = (size_t)S * S;
  if (out_rgb) {
    if (normalize) {                                                   // rgb_transform after the crop: the padding too
      r = (r - m0) / s0;
      g = (g - m1) / s1;
      b = (b - m2) / s2;
    }
    float *d = out_rgb + (size_t)t * 3 * plane + o;
    d[0] = r;
    d[plane] = g;
    d[2 * plane] = b;
  }
  if (out_mask) out_mask[(size_t)t * plane + o] = mk;
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
  hipLaunchKernelGGL(template_pem_crops_kernel, dim3((unsigned)g), dim3(256), 0, as_stream(stream), images, mask,
                     (const long *)box, T, H, W, S, use_mask, mean3_host[0], mean3_host[1], mean3_host[2], std3_host[0],
                     std3_host[1], std3_host[2], out);
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
