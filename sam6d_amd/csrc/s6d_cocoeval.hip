// hipcc-flags: -ffp-contract=off
// COCO detection / segmentation AP of ISM results on the device (gfx950): bit-packed masks, their pairwise intersections, box IoUs
// and the greedy matching.  pycocotools and bop_toolkit are not part of this project and none of their text is used: the quantities
// are DEFINED in sam6d_amd/evaluation.py (and DESIGN section 12), operation by operation, and the tests pin these kernels to an
// independent restatement of that definition (tests/coco_ref.py).  Nothing claims equality with another tool's output.
//
// mask_pack_kernel        masks (N, HW) bytes, a pixel is set when its byte is not 0 -> packed (N, words) 64-bit words, words =
//                         ceil(HW / 64): bit k of word j is pixel 64 j + k (row-major pixel order), the bits past HW are 0; area[n]
//                         = the number of set pixels.  A wave makes PK_WORDS consecutive words of one mask: lane l reads pixel
//                         64 j + l (64 consecutive bytes per wave instruction, any alignment), one __ballot per word, the words
//                         stored by the first PK_WORDS lanes in one instruction, one integer atomicAdd of the popcounts per wave into
//                         the zeroed areas.
// mask_pair_inter_kernel  pairs (P, 2) = (row of dpacked, row of gpacked) -> inter[p] = popcount(d & g).  The grid is (P, chunks), a
//                         chunk = CE_CHUNK words.  The pair list is cut into SEGMENTS of consecutive pairs with the same detection
//                         row: a pair p is the head of a segment when p = 0, or its detection row differs from pair p - 1's, or p is
//                         a multiple of CE_RUN and the same row goes back at least CE_RUN pairs (so a segment has at most
//                         2 CE_RUN - 1 pairs, and a run shorter than CE_RUN -- a detection against the ground truths of its group --
//                         is ONE segment).  The workgroup of a head keeps its chunk of the detection row in registers (CE_WPL words
//                         per lane, read once) and walks the segment's ground-truth rows with 8-byte loads, __popcll, a wave sum
//                         (shuffles) and the four waves through LDS; the workgroups of the other pairs leave at once.  One integer
//                         atomicAdd per (pair, chunk) into the zeroed output: integer sums do not depend on their order, so a pair
//                         has the same count under any P, any pair order and any segmentation.  A row index outside its array
//                         leaves the pair's count 0 (the wrapper refuses it on the host).
// box_pair_iou_kernel     one lane per pair, float64, boxes x y w h:  w = min(dx + dw, gx + gw) - max(dx, gx), h likewise; 0 when
//                         w <= 0 or h <= 0; else i = w h, u = (dw dh + gw gh) - i, iou = i / u -- every product and sum rounded on
//                         its own (contraction is off for the whole file: the first line), one IEEE division.
// coco_match_kernel       one workgroup (one wave) per group = (image, category); lane = threshold * NA + area range, 40 of the 64
//                         lanes for the 10 x 4 of the definition.  The lane walks the group's detections in the given (score) order
//                         against its G <= 64 ground truths, the matched ones held in one 64-bit mask:
//                           bar = min(t, 1 - 1e-10); over the unmatched, non-ignored ground truths in input order an IoU >= bar takes
//                           the match and becomes the bar (so of equal IoUs the later wins); only when none matched the same walk
//                           over the ignored ones.  A ground truth is ignored in a range when it is flagged or its area is outside
//                           [lo, hi]; a detection is ignored when its match is, or when it has none and its own area is outside.
//                         -> match (D, NT, NA) int32 = the ground truth's index inside the group or -1, ignore (D, NT, NA) bytes.
//                         A group whose table row does not fit the arrays (or G > 64) is left at -1 / 0: the wrapper refuses it.
#include "s6d_common.h"

namespace s6d {

#pragma clang fp contract(off)   // the stated float64 operations, one rounding each

typedef unsigned long long u64;

constexpr int CE_THREADS = 256;
constexpr int CE_WAVES = CE_THREADS / kWave;
constexpr int PK_WORDS = 8;                                              // words of one wave
constexpr int PK_BLOCK_WORDS = PK_WORDS * CE_WAVES;                      // words of one workgroup
constexpr int CE_WPL = 8;                                                // detection words a lane keeps
constexpr int CE_CHUNK = CE_THREADS * CE_WPL;                            // words of one workgroup
constexpr int CE_RUN = 64;                                               // a same-row run is cut at multiples of this
constexpr int CM_MAX_GT = 64;
constexpr int CM_LANES = 64;

__global__ __launch_bounds__(CE_THREADS) void mask_pack_kernel(const uint8_t *__restrict__ masks, long HW, int words, int blocks,
                                                               u64 *__restrict__ packed, int *__restrict__ area) {
  const int n = blockIdx.x / blocks, blk = blockIdx.x - n * blocks;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int j0 = (blk * CE_WAVES + wave) * PK_WORDS;
  const uint8_t *M = masks + (size_t)n * HW;
  uint8_t v[PK_WORDS];
#pragma unroll
  for (int k = 0; k < PK_WORDS; ++k) {
    const long pix = (long)(j0 + k) * 64 + lane;
    v[k] = pix < HW ? M[pix] : (uint8_t)0;                               // (a word past the row has no pixel below HW either)
  }
  u64 mine = 0;
  int cnt = 0;
#pragma unroll
  for (int k = 0; k < PK_WORDS; ++k) {
    const u64 b = __ballot(v[k] != 0);
    cnt += __popcll(b);
    if (lane == k) mine = b;
  }
  if (lane < PK_WORDS && j0 + lane < words) packed[(size_t)n * words + j0 + lane] = mine;
  if (lane == 0 && cnt != 0) atomicAdd(&area[n], cnt);
}

__global__ __launch_bounds__(CE_THREADS) void mask_pair_inter_kernel(const u64 *__restrict__ dpacked, int Nd,
                                                                     const u64 *__restrict__ gpacked, int Ng, long words,
                                                                     const int *__restrict__ pairs, int P, int *__restrict__ inter) {
  __shared__ int red[2 * CE_RUN][CE_WAVES];
  const int p = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int d = pairs[2 * (size_t)p];
  int start = p;                                                         // (a lower bound of) where this detection row's run begins
  if (p != 0 && pairs[2 * (size_t)(p - 1)] == d) {
    if (p % CE_RUN != 0) return;                                         // the whole workgroup, here and below
    const int q = p - 1 - lane;                                          // p >= CE_RUN: q >= 0
    const bool begins = lane < CE_RUN - 1 && (q == 0 || pairs[2 * (size_t)(q - 1)] != pairs[2 * (size_t)q]);
    if (__ballot(begins) != 0) return;                                   // the run began less than CE_RUN pairs back: not a head
    start = p - CE_RUN;
  }
  int end = p + 1;
  while (end < P && pairs[2 * (size_t)end] == d && !(end % CE_RUN == 0 && end >= start + CE_RUN)) ++end;
  const int n = end - p;                                                 // <= 2 CE_RUN - 1
  if (d < 0 || d >= Nd) return;
  const long w0 = (long)blockIdx.y * CE_CHUNK + threadIdx.x;
  const u64 *D = dpacked + (size_t)d * words;
  u64 dw[CE_WPL];
#pragma unroll
  for (int k = 0; k < CE_WPL; ++k) {
    const long w = w0 + (long)k * CE_THREADS;
    dw[k] = w < words ? D[w] : 0ull;
  }
  for (int j = 0; j < n; ++j) {
    const int g = pairs[2 * (size_t)(p + j) + 1];
    int c = 0;
    if (g >= 0 && g < Ng) {
      const u64 *G = gpacked + (size_t)g * words;
      u64 gw[CE_WPL];
#pragma unroll
      for (int k = 0; k < CE_WPL; ++k) {
        const long w = w0 + (long)k * CE_THREADS;
        gw[k] = w < words ? G[w] : 0ull;
      }
#pragma unroll
      for (int k = 0; k < CE_WPL; ++k) c += __popcll(dw[k] & gw[k]);
    }
    c = wave_sum_i32(c);
    if (lane == 0) red[j][wave] = c;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < n; j += CE_THREADS) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < CE_WAVES; ++w) s += red[j][w];
    if (s != 0) atomicAdd(&inter[p + j], s);
  }
}

__global__ __launch_bounds__(CE_THREADS) void box_pair_iou_kernel(const double *__restrict__ dboxes, int Nd,
                                                                  const double *__restrict__ gboxes, int Ng,
                                                                  const int *__restrict__ pairs, int P, double *__restrict__ iou) {
  const long p = (long)blockIdx.x * CE_THREADS + threadIdx.x;
  if (p >= P) return;
  const int d = pairs[2 * p], g = pairs[2 * p + 1];
  double r = 0.0;
  if (d >= 0 && d < Nd && g >= 0 && g < Ng) {
    const double dx = dboxes[4 * (size_t)d], dy = dboxes[4 * (size_t)d + 1], dw = dboxes[4 * (size_t)d + 2], dh = dboxes[4 * (size_t)d + 3];
    const double gx = gboxes[4 * (size_t)g], gy = gboxes[4 * (size_t)g + 1], gw = gboxes[4 * (size_t)g + 2], gh = gboxes[4 * (size_t)g + 3];
    // plain operators: contraction is off for this file (the first line) and for this namespace (the pragma), so each is one
    // rounding.  (__dmul_rn / __dadd_rn are inline `x * y` / `x + y` of a header compiled under the default contraction: their
    // results DID fuse into v_fma_f64 here.)
    const double w = fmin(dx + dw, gx + gw) - fmax(dx, gx);
    const double h = fmin(dy + dh, gy + gh) - fmax(dy, gy);
    if (w > 0.0 && h > 0.0) {
      const double i = w * h;
      const double a = dw * dh;
      const double b = gw * gh;
      const double u = (a + b) - i;
      r = i / u;
    }
  }
  iou[p] = r;
}

__global__ __launch_bounds__(CM_LANES) void coco_match_kernel(const double *__restrict__ ious, const long *__restrict__ iou_off,
                                                              const int *__restrict__ groups, const double *__restrict__ det_area,
                                                              const double *__restrict__ gt_area, const uint8_t *__restrict__ gt_ignore,
                                                              const double *__restrict__ params, int NT, int NA, long n_det,
                                                              long n_gt, long n_iou, int *__restrict__ match,
                                                              uint8_t *__restrict__ ignore) {
  const int grp = blockIdx.x, lane = threadIdx.x;
  const long d0 = groups[4 * (size_t)grp], D = groups[4 * (size_t)grp + 1], g0 = groups[4 * (size_t)grp + 2];
  const int G = groups[4 * (size_t)grp + 3];
  const long i0 = iou_off[grp];
  if (d0 < 0 || D < 0 || g0 < 0 || G < 0 || G > CM_MAX_GT || i0 < 0 || d0 + D > n_det || g0 + G > n_gt || i0 + D * G > n_iou) return;
  if (lane >= NT * NA) return;
  const int t = lane / NA, a = lane - t * NA;
  const double thr = fmin(params[t], 1.0 - 1e-10);
  const double lo = params[NT + 2 * a], hi = params[NT + 2 * a + 1];
  u64 ign = 0, taken = 0;
  for (int g = 0; g < G; ++g) {
    const double ar = gt_area[g0 + g];
    if (gt_ignore[g0 + g] != 0 || ar < lo || ar > hi) ign |= 1ull << g;
  }
  const u64 all = G == 64 ? ~0ull : (1ull << G) - 1ull;
  for (long d = 0; d < D; ++d) {
    const double *row = ious + i0 + d * G;
    double bar = thr;
    int m = -1;
#pragma unroll 1
    for (int pass = 0; pass < 2 && m < 0; ++pass) {
      const u64 open = all & ~taken & (pass == 0 ? ~ign : ign);
      for (int g = 0; g < G; ++g) {
        if (!((open >> g) & 1ull)) continue;
        const double v = row[g];
        if (v < bar) continue;
        bar = v;
        m = g;
      }
    }
    bool ig;
    if (m >= 0) {
      taken |= 1ull << m;
      ig = (ign >> m) & 1ull;
    } else {
      const double ar = det_area[d0 + d];
      ig = ar < lo || ar > hi;
    }
    const size_t o = (size_t)(d0 + d) * (NT * NA) + lane;
    match[o] = m;
    ignore[o] = ig ? 1 : 0;
  }
}

static int clear_async(void *p, int value, size_t bytes, hipStream_t s) {
  const hipError_t e = hipMemsetAsync(p, value, bytes, s);
  if (e != hipSuccess) {
    set_hip_error(e);
    return S6D_ELAUNCH;
  }
  return S6D_OK;
}

}  // namespace s6d

using namespace s6d;

extern "C" int s6d_mask_pack_u8(const uint8_t *masks, int N, long HW, uint64_t *packed, int32_t *area, void *stream) {
  if (N < 0 || HW < 1) return S6D_EINVAL;
  if (HW > 0x7fffffffL) return S6D_EUNSUPPORTED;
  const long words = (HW + 63) / 64, blocks = (words + PK_BLOCK_WORDS - 1) / PK_BLOCK_WORDS;
  if ((long)N * blocks > 0x7fffffffL) return S6D_EUNSUPPORTED;
  if (N == 0) return S6D_OK;
  if (!masks || !packed || !area) return S6D_EINVAL;
  hipStream_t s = as_stream(stream);
  const int rc = clear_async(area, 0, (size_t)N * 4, s);
  if (rc != S6D_OK) return rc;
  hipLaunchKernelGGL(mask_pack_kernel, dim3((unsigned)((long)N * blocks)), dim3(CE_THREADS), 0, s, masks, HW, (int)words, (int)blocks,
                     reinterpret_cast<u64 *>(packed), area);
  return launch_status();
}

extern "C" int s6d_mask_pair_inter(const uint64_t *dpacked, int Nd, const uint64_t *gpacked, int Ng, long words, const int32_t *pairs,
                                   int P, int32_t *inter, void *stream) {
  if (Nd < 0 || Ng < 0 || words < 1 || P < 0) return S6D_EINVAL;
  const long chunks = (words + CE_CHUNK - 1) / CE_CHUNK;
  if (chunks > 65535 || words * 64 > 0x7fffffffL) return S6D_EUNSUPPORTED;    // (counts are int32)
  if (P == 0) return S6D_OK;
  if (Nd == 0 || Ng == 0) return S6D_EINVAL;                                // pairs into an empty array
  if (!dpacked || !gpacked || !pairs || !inter) return S6D_EINVAL;
  hipStream_t s = as_stream(stream);
  const int rc = clear_async(inter, 0, (size_t)P * 4, s);
  if (rc != S6D_OK) return rc;
  hipLaunchKernelGGL(mask_pair_inter_kernel, dim3((unsigned)P, (unsigned)chunks), dim3(CE_THREADS), 0, s,
                     reinterpret_cast<const u64 *>(dpacked), Nd, reinterpret_cast<const u64 *>(gpacked), Ng, words, pairs, P, inter);
  return launch_status();
}

extern "C" int s6d_box_pair_iou_f64(const double *dboxes, int Nd, const double *gboxes, int Ng, const int32_t *pairs, int P,
                                    double *iou, void *stream) {
  if (Nd < 0 || Ng < 0 || P < 0) return S6D_EINVAL;
  if (P == 0) return S6D_OK;
  if (Nd == 0 || Ng == 0) return S6D_EINVAL;
  if (!dboxes || !gboxes || !pairs || !iou) return S6D_EINVAL;
  hipLaunchKernelGGL(box_pair_iou_kernel, dim3((unsigned)(((long)P + CE_THREADS - 1) / CE_THREADS)), dim3(CE_THREADS), 0,
                     as_stream(stream), dboxes, Nd, gboxes, Ng, pairs, P, iou);
  return launch_status();
}

extern "C" int s6d_coco_match(const double *ious, const long *iou_off, const int32_t *groups, const double *det_area,
                              const double *gt_area, const uint8_t *gt_ignore, const double *params, int n_groups, int NT, int NA,
                              long n_det, long n_gt, long n_iou, int32_t *match, uint8_t *ignore, void *stream) {
  if (n_groups < 0 || NT < 1 || NA < 1 || NT * (long)NA > CM_LANES || n_det < 0 || n_gt < 0 || n_iou < 0) return S6D_EINVAL;
  if (n_groups == 0 || n_det == 0) return S6D_OK;
  if (!iou_off || !groups || !det_area || !params || !match || !ignore) return S6D_EINVAL;
  if ((n_gt > 0 && (!gt_area || !gt_ignore)) || (n_iou > 0 && !ious)) return S6D_EINVAL;
  hipStream_t s = as_stream(stream);
  int rc = clear_async(match, 0xff, (size_t)n_det * NT * NA * 4, s);     // every byte 0xff: -1
  if (rc == S6D_OK) rc = clear_async(ignore, 0, (size_t)n_det * NT * NA, s);
  if (rc != S6D_OK) return rc;
  hipLaunchKernelGGL(coco_match_kernel, dim3((unsigned)n_groups), dim3(CM_LANES), 0, s, ious, iou_off, groups, det_area, gt_area,
                     gt_ignore, params, NT, NA, n_det, n_gt, n_iou, match, ignore);
  return launch_status();
}
