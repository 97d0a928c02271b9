// Kernels of the PEM per-detection pre-processing (host side: sam6d_amd/pem/preprocess.py).
//
//   sample_indices   the point sampler of get_test_data / get_instance (Pose_Estimation_Model/run_inference_custom.py:224-229,
//                    provider/bop_test_dataset.py:140-145) in its DEFINED form (preprocess.py header: injected uniforms
//                    instead of numpy's global RNG): per detection with n candidate points and keys u_0 .. u_{n-1},
//                      n <= n_sample : idx_i = floor(u_i * n) for i < n_sample            (with replacement)
//                      n >  n_sample : the positions of the n_sample smallest (u, position) pairs, ascending
//                                      (without replacement; == the first n_sample entries of a stable argsort).
//                    The library version is one top-k over a (P, L) table of 64-bit composite keys -- a full sort of up to
//                    3e5 entries per detection.  Here one workgroup per detection reads its keys twice: a 4096-bin histogram of
//                    the keys' leading bits finds the bin in which the n_sample-th smallest key lies, the (at most 4096) keys
//                    up to that bin are collected in LDS and sorted there (bitonic, 64-bit composite key << 32 | position).
//                    Exact, deterministic, independent of the order of the atomics.  Keys must be non-negative floats (their
//                    bit patterns then order like their values); if more than 4096 keys share the leading bits up to the
//                    threshold bin (heavily duplicated keys, never uniform ones) the detection is flagged in `overflow` and the
//                    caller uses the library path for it.  (n_sample > 2048, the 5000 points of a template view: the same kernel
//                    with 8192 candidates, kSelCapBig below.)
//   compact_cloud    "mask -> choose -> cloud" of get_test_data (:209-213): the masked pixels of a detection's square crop in
//                    row-major crop order (``mask[y1:y2, x1:x2].flatten().nonzero()``) with their back-projected points
//                    (utils/data_utils.py:92-110: x = (u - cx) z / fx, y = (v - cy) z / fy in float32, that operation order).
//                    The library version builds ONE list for the frame with nonzero + five boolean-mask indexings (a host round
//                    trip each).  Here one workgroup per detection walks its crop in chunks of 1024 pixels and compacts in
//                    order (wave ballot ranks + a 16-entry wave prefix), writing to the detection's fixed-capacity slot.
//   radius_filter    ``flag = norm(cloud - center) < radius * 1.2`` (:214-221) and the second in-order compaction, in place.
//   crops            the masked colour crop of every surviving detection (:229-236): pem_crops_kernel<FrameCrops> of s6d_cv_resize.h.
// The template twin is s6d_onboard.hip.  The two share, each written once: the count / extent reduction and the crop walk with its
// compaction (s6d_compact.h), get_bbox (s6d_crop_params.h), the colour crop kernel (s6d_cv_resize.h).  Guards of both: a box that
// does not lie inside the frame, or holds more than cap pixels, compacts to n = 0 with nothing written; its colour crop is that of a
// black crop, (0 - mean) / std.  kept[k] is not checked.
#include "s6d_common.h"
#include "s6d_compact.h"
#include "s6d_crop_params.h"
#include "s6d_cv_resize.h"

namespace s6d {

#pragma clang fp contract(off)   // the reference's float32 expressions, operation by operation (no fused multiply-adds)

// mask (P,H,W) u8 (non-zero = set), depth (H,W) f32 -> m (P,H,W) u8 = mask AND depth > 0, cnt (P) i64, ok (P) u8 = cnt > min_points,
// box (P,4) i64: get_bbox (utils/data_utils.py:126-160) of m -- of the whole frame for a detection that is not ok, like the
// library path's dummy mask.  One workgroup per detection, one pass over its mask.
__global__ __launch_bounds__(kCmpThreads) void mask_boxes_kernel(const unsigned char *__restrict__ mask,
                                                                const float *__restrict__ depth, int H, int W, long min_points,
                                                                unsigned char *__restrict__ m, long *__restrict__ cnt_out,
                                                                unsigned char *__restrict__ ok_out, long *__restrict__ box) {
  const int p = blockIdx.x, tid = threadIdx.x;
  const size_t off = (size_t)p * H * W;
  int cnt = 0, b[4];
  extent_init(b, H, W);
  for (int i = tid; i < H * W; i += kCmpThreads) {
    const bool v = mask[off + i] != 0 && depth[i] > 0.f;
    m[off + i] = v ? 1 : 0;
    if (v) {
      const int y = i / W;
      ++cnt;
      extent_add(b, y, i - y * W);
    }
  }
  const long c = block_extents<1>(cnt, b);
  if (tid == 0) {
    const bool ok = c > min_points;
    cnt_out[p] = c;
    ok_out[p] = ok ? 1 : 0;
    extent_box(ok, b, H, W, box + p * 4);
  }
}

// m (P,H,W) u8 = mask AND depth > 0; box (P,4) i64 [y1,y2,x1,x2]; ok (P) u8 -> choose (P,cap) i32, cloud (P,cap,3) f32, n (P) i64
__global__ __launch_bounds__(kCmpThreads) void compact_cloud_kernel(const unsigned char *__restrict__ m,
                                                                   const float *__restrict__ depth,
                                                                   const long *__restrict__ box,
                                                                   const unsigned char *__restrict__ ok, int H, int W,
                                                                   float fx, float fy, float cx, float cy, long cap,
                                                                   int *__restrict__ choose, float *__restrict__ cloud,
                                                                   long *__restrict__ n_out) {
  const int p = blockIdx.x;
  const unsigned char *mp = m + (size_t)p * H * W;
  compact_crop(
      box + p * 4, ok[p] != 0, H, W, cap, n_out + p, [&](int pix) { return mp[pix] != 0; },
      [&](long pos, int j, int y, int x) {
        const float z = depth[y * W + x];
        choose[(size_t)p * cap + pos] = j;
        float *c = cloud + ((size_t)p * cap + pos) * 3;
        c[0] = ((float)x - cx) * z / fx;
        c[1] = ((float)y - cy) * z / fy;
        c[2] = z;
      });
}

// in place: keep the points within lim[p] of center[p], in order.  choose (P,cap) i32, cloud (P,cap,3) f32, n (P) i64 in/out
__global__ __launch_bounds__(kCmpThreads) void radius_filter_kernel(const float *__restrict__ center,
                                                                   const double *__restrict__ lim, long cap,
                                                                   int *__restrict__ choose, float *__restrict__ cloud,
                                                                   long *__restrict__ n_io) {
  __shared__ unsigned wave_tot[kCmpThreads / 64];
  __shared__ long base;
  const int p = blockIdx.x, tid = threadIdx.x;
  const long n = n_io[p];
  if (tid == 0) base = 0;
  __syncthreads();
  const float c0 = center[p * 3 + 0], c1 = center[p * 3 + 1], c2 = center[p * 3 + 2];
  const double limit = lim[p];
  int *ch = choose + (size_t)p * cap;
  float *cl = cloud + (size_t)p * cap * 3;
  for (long s0 = 0; s0 < n; s0 += kCmpThreads) {
    const long i = s0 + tid;
    bool keep = false;
    float vx = 0.f, vy = 0.f, vz = 0.f;
    int cj = 0;
    if (i < n) {
      vx = cl[i * 3 + 0];
      vy = cl[i * 3 + 1];
      vz = cl[i * 3 + 2];
      cj = ch[i];
      const float dx = vx - c0, dy = vy - c1, dz = vz - c2;
      const float d = sqrtf((dx * dx + dy * dy) + dz * dz);
      keep = (double)d < limit;
    }
    const long pos = block_rank(keep, &base, wave_tot);   // its barriers also order this chunk's reads before the writes below
    if (keep) {                                           // pos <= i: never overwrites an element that is still to be read
      ch[pos] = cj;
      cl[pos * 3 + 0] = vx;
      cl[pos * 3 + 1] = vy;
      cl[pos * 3 + 2] = vz;
    }
  }
  __syncthreads();
  if (tid == 0) n_io[p] = base;
}

constexpr int kSelThreads = 1024;
constexpr int kSelBins = 4096;        // leading 12 bits of the float (sign is 0: 8 exponent + 3 mantissa bits ... see below)
constexpr int kSelCap = 4096;         // candidates sorted in LDS (32 KB of 64-bit composites): n_sample <= 2048
// n_sample up to kSelMaxSample (the 5000 points of a template view, run_inference_custom.py:138-141): the threshold bin is at most
// 1/16 of the key range below it wide, so uniform keys put about n_sample * 17/16 candidates in front of the sort; 8192 composites
// are 64 KiB, with the histogram 80 KiB of the CU's 160 KiB LDS -- one workgroup per CU, which 1024 threads allow anyway
constexpr int kSelCapBig = 8192;
constexpr int kSelMaxSample = 6144;

// bin of a non-negative float: its 12 leading bits below the sign (exponent + 4 mantissa bits)
__device__ __forceinline__ unsigned sel_bin(unsigned bits) {
  const unsigned b = bits >> 19;
  return b < (unsigned)kSelBins ? b : (unsigned)kSelBins - 1;    // negative / NaN keys are outside the contract; no wild index
}

template <int kCap>
__global__ __launch_bounds__(kSelThreads) void sample_indices_kernel(const float *__restrict__ keys, long key_stride,
                                                                    const long *__restrict__ count, int n_sample,
                                                                    long *__restrict__ idx, int *__restrict__ overflow) {
  __shared__ unsigned hist[kSelBins];
  __shared__ unsigned long long cand[kCap];
  __shared__ unsigned s_thr, s_ncand;
  const int p = blockIdx.x, tid = threadIdx.x;
  const long n = count[p];
  const float *k = keys + (size_t)p * key_stride;
  long *out = idx + (size_t)p * n_sample;
  if (n <= n_sample) {                                   // with replacement (also n == 0: every index 0)
    for (int i = tid; i < n_sample; i += kSelThreads) out[i] = (long)floor((double)k[i] * (double)n);
    if (tid == 0) overflow[p] = 0;
    return;
  }
  for (int i = tid; i < kSelBins; i += kSelThreads) hist[i] = 0;
  if (tid == 0) s_ncand = 0;
  __syncthreads();
  for (long i = tid; i < n; i += kSelThreads) atomicAdd(&hist[sel_bin(__float_as_uint(k[i]))], 1u);
  __syncthreads();
  if (tid == 0) {                                        // the bin holding the n_sample-th smallest key
    unsigned cum = 0, t = 0;
    for (; t < kSelBins; ++t) {
      cum += hist[t];
      if (cum >= (unsigned)n_sample) break;
    }
    s_thr = t;
    if (cum > (unsigned)kCap) s_ncand = 0xffffffffu;  // too many keys up to the threshold bin for the LDS sort
  }
  __syncthreads();
  const unsigned thr = s_thr;
  if (s_ncand == 0xffffffffu) {
    if (tid == 0) overflow[p] = 1;
    return;
  }
  for (int i = tid; i < kCap; i += kSelThreads) cand[i] = ~0ull;
  __syncthreads();
  for (long i = tid; i < n; i += kSelThreads) {
    const unsigned b = __float_as_uint(k[i]);
    if (sel_bin(b) <= thr) cand[atomicAdd(&s_ncand, 1u)] = ((unsigned long long)b << 32) | (unsigned long long)i;
  }
  __syncthreads();
  // bitonic sort of kCap 64-bit composites, ascending (the padding ~0 sorts last)
  for (int size = 2; size <= kCap; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < kCap / 2; t += kSelThreads) {
        const int lo = 2 * t - (t & (stride - 1));        // index of the lower element of pair t at this stride
        const int hi = lo + stride;
        const bool up = (lo & size) == 0;
        const unsigned long long a = cand[lo], c = cand[hi];
        if ((a > c) == up) {
          cand[lo] = c;
          cand[hi] = a;
        }
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < n_sample; i += kSelThreads) out[i] = (long)(cand[i] & 0xffffffffull);
  if (tid == 0) overflow[p] = 0;
}

}  // namespace s6d

using namespace s6d;

extern "C" int s6d_pem_sample_indices_f32(const float *keys, long key_stride, const int64_t *count, int P, int n_sample,
                                          int64_t *idx, int32_t *overflow, void *stream) {
  if (P < 0 || n_sample <= 0 || n_sample > kSelMaxSample || key_stride < n_sample) return S6D_EINVAL;
  if (P == 0) return S6D_OK;
  if (!keys || !count || !idx || !overflow) return S6D_EINVAL;
  if (n_sample <= kSelCap / 2)                           // the kernel these sizes have always had: the same bits, the same flag
    hipLaunchKernelGGL(sample_indices_kernel<kSelCap>, dim3((unsigned)P), dim3(kSelThreads), 0, as_stream(stream), keys, key_stride,
                       (const long *)count, n_sample, (long *)idx, overflow);
  else
    hipLaunchKernelGGL(sample_indices_kernel<kSelCapBig>, dim3((unsigned)P), dim3(kSelThreads), 0, as_stream(stream), keys,
                       key_stride, (const long *)count, n_sample, (long *)idx, overflow);
  return launch_status();
}

extern "C" int s6d_pem_compact_cloud_f32(const unsigned char *m, const float *depth, const int64_t *box, const unsigned char *ok,
                                         int P, int H, int W, float fx, float fy, float cx, float cy, long cap, int32_t *choose,
                                         float *cloud, int64_t *n, void *stream) {
  if (P < 0 || H <= 0 || W <= 0 || (long)H * W > 0x7fffffffL || cap <= 0 || fx == 0.f || fy == 0.f) return S6D_EINVAL;
  if (P == 0) return S6D_OK;
  if (!m || !depth || !box || !ok || !choose || !cloud || !n) return S6D_EINVAL;
  hipLaunchKernelGGL(compact_cloud_kernel, dim3((unsigned)P), dim3(kCmpThreads), 0, as_stream(stream), m, depth,
                     (const long *)box, ok, H, W, fx, fy, cx, cy, cap, choose, cloud, (long *)n);
  return launch_status();
}

extern "C" int s6d_pem_radius_filter_f32(const float *center, const double *limit, int P, long cap, int32_t *choose,
                                         float *cloud, int64_t *n, void *stream) {
  if (P < 0 || cap <= 0) return S6D_EINVAL;
  if (P == 0) return S6D_OK;
  if (!center || !limit || !choose || !cloud || !n) return S6D_EINVAL;
  hipLaunchKernelGGL(radius_filter_kernel, dim3((unsigned)P), dim3(kCmpThreads), 0, as_stream(stream), center, limit, cap,
                     choose, cloud, (long *)n);
  return launch_status();
}

extern "C" int s6d_pem_mask_boxes_u8(const unsigned char *mask, const float *depth, int P, int H, int W, long min_points,
                                     unsigned char *m, int64_t *cnt, unsigned char *ok, int64_t *box, void *stream) {
  if (P < 0 || H <= 0 || W <= 0 || (long)H * W > 0x7fffffffL) return S6D_EINVAL;
  if (P == 0) return S6D_OK;
  if (!mask || !depth || !m || !cnt || !ok || !box) return S6D_EINVAL;
  hipLaunchKernelGGL(mask_boxes_kernel, dim3((unsigned)P), dim3(kCmpThreads), 0, as_stream(stream), mask, depth, H, W, min_points,
                     m, (long *)cnt, ok, (long *)box);
  return launch_status();
}

extern "C" int s6d_pem_crops_f32(const unsigned char *image, const unsigned char *m, const int64_t *kept, const int64_t *box,
                                 int M, int H, int W, int S, int use_mask, const float *mean3_host, const float *std3_host,
                                 float *out, void *stream) {
  if (M < 0 || H <= 0 || W <= 0 || S <= 0 || (long)H * W > 0x7fffffffL) return S6D_EINVAL;
  if (M == 0) return S6D_OK;
  if (!image || !m || !kept || !box || !mean3_host || !std3_host || !out) return S6D_EINVAL;
  const size_t total = (size_t)M * 3 * S * S;
  size_t g = (total + 255) / 256;
  if (g > 16384) g = 16384;
  const FrameCrops src{image, m, (const long *)kept};
  hipLaunchKernelGGL(pem_crops_kernel<FrameCrops>, dim3((unsigned)g), dim3(256), 0, as_stream(stream), src, (const long *)box, M, H,
                     W, S, use_mask, mean3_host[0], mean3_host[1], mean3_host[2], std3_host[0], std3_host[1], std3_host[2], out);
  return launch_status();
}
