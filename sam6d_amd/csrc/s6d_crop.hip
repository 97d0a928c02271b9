// Proposal crops for the DINOv2 descriptor model, fused (gfx950): normalise . mask . crop . nearest-resize . zero-pad .
// nearest-resize in one pass -- one read of the frame / mask pixels that survive, one write of the crop.
//
// Reference: CustomDINOv2.process_rgb_proposals / process_masks_proposals (Instance_Segmentation_Model/model/
// dinov2.py:131-144, 178-189) = rgb_normalize (ToTensor + Normalize), an (P,3,H,W) repeat * mask, then
// CropResizePad.__call__ (utils/bbox_utils.py:98-126): a per-proposal Python loop of slice, F.interpolate(nearest,
// scale_factor), F.pad, F.interpolate(nearest, scale_factor).  The host side (sam6d_amd/ism/dinov2.py) mirrors the
// loop's double-precision size arithmetic and hands every proposal's geometry over as one CropParams record; the
// kernel mirrors ATen's nearest index rule (UpSample.h nearest_neighbor_compute_source_index, the one the CUDA kernel
// and the CPU generic kernel use): src = min(floorf(dst * float(1 / scale)), in - 1) with the USER scale_factor, not
// out / in -- also when out == in (a 17-wide crop "resized" by 1.04 to 17 columns repeats column 0 and drops 16).
// That geometry (crop_src) and the three-plane store are s6d_crop_params.h's, shared with the template crops of s6d_onboard.hip,
// which differ in the pixel arithmetic alone; a record whose source pixel lies outside the frame gives padding (rgb 0, mask 0).
#include "s6d_common.h"
#include "s6d_crop_params.h"

namespace s6d {

__global__ __launch_bounds__(256) void crop_resize_pad_kernel(const unsigned char *__restrict__ image,
                                                              const float *__restrict__ masks,
                                                              const CropParams *__restrict__ params, int P, int H, int W,
                                                              int T, float m0, float m1, float m2, float s0, float s1,
                                                              float s2, float *__restrict__ out_rgb,
                                                              float *__restrict__ out_mask) {
  const int p = blockIdx.y;
  const int o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= T * T) return;
  int sy, sx;
  float r = 0.f, g = 0.f, b = 0.f, mk = 0.f;
  if (crop_src(params[p], o, T, H, W, sy, sx)) {
    const size_t pix = (size_t)sy * W + sx;
    mk = masks[(size_t)p * H * W + pix];
    if (out_rgb) {
      const unsigned char *q = image + pix * 3;
      // ToTensor (/255), Normalize ((x - mean) / std), then * mask: the reference's three roundings, in its order
      r = (((float)q[0] / 255.0f - m0) / s0) * mk;
      g = (((float)q[1] / 255.0f - m1) / s1) * mk;
      b = (((float)q[2] / 255.0f - m2) / s2) * mk;
    }
  }
  if (out_rgb) store_rgb_planes(out_rgb + (size_t)p * 3 * T * T, o, T, r, g, b);
  if (out_mask) out_mask[(size_t)p * T * T + o] = mk;
}

}  // namespace s6d

using namespace s6d;

extern "C" int s6d_crop_resize_pad_f32(const unsigned char *image, const float *masks, const void *params, int P, int H,
                                       int W, int T, const float *mean3_host, const float *std3_host, float *out_rgb,
                                       float *out_mask, void *stream) {
  if (P < 0 || H <= 0 || W <= 0 || T <= 0 || (long)H * W > 0x7fffffffL) return S6D_EINVAL;
  if (P == 0) return S6D_OK;
  if (!masks || !params || (!out_rgb && !out_mask) || (out_rgb && (!image || !mean3_host || !std3_host)))
    return S6D_EINVAL;
  const float one[3] = {1.f, 1.f, 1.f}, zero[3] = {0.f, 0.f, 0.f};
  const float *m = out_rgb ? mean3_host : zero, *s = out_rgb ? std3_host : one;
  const dim3 grid((unsigned)((T * T + 255) / 256), (unsigned)P);
  hipLaunchKernelGGL(crop_resize_pad_kernel, grid, dim3(256), 0, as_stream(stream), image, masks,
                     (const CropParams *)params, P, H, W, T, m[0], m[1], m[2], s[0], s[1], s[2], out_rgb, out_mask);
  return launch_status();
}
