// Pose verification against the measured depth on the device (gfx950): per-pose evidence counts from the rendered and the measured
// depth, and a scene-level selection in which a measured pixel supports at most one accepted pose.  SAM-6D has no such step and no
// other tool's hypothesis verification is restated: the step is DEFINED here, operation by operation, and the tests pin the kernels
// to an independent restatement of this header in plain loops (tests/verify_ref.py).  All of it is integer work after two float32
// operations per pixel: the result is exact and does not depend on the batch, the chunking or the scheduling.
//
// EVIDENCE (verify_evidence_kernel), instance n at row-major pixel p of H W:
//   r          render[n][p]: camera Z of the instance at its pose in model units, 0 on background (s6d_raster_depth_f32).
//   rendered   r > 0 (NaN fails).
//   z          depth_obs[obs_index[n]][p] * depth_unit: ONE float32 multiply.
//   measured   0 < z < +inf (NaN fails).
//   d          z - r: ONE float32 subtraction; the multiply and the subtraction are never contracted into a fused operation.
//   class      a rendered pixel is exactly one of  MISSING  not measured;  INLIER  |d| <= tau;  OCCLUDED  d < -tau (something
//              nearer was measured);  BEHIND  d > tau (the camera sees through the model).  (d is never NaN: z is finite, r > 0.)
//   det        masks[n][p] != 0; without masks (NULL) false.
//   counts     (N,8) int32 = rendered, missing, inlier, occluded, behind, det, det && rendered, det && inlier.
//   inlier     (N, ceil(H W / 64)) words in the layout of s6d_mask_pack_u8: bit k of word j is pixel 64 j + k, tail bits zero.
//   span       (N,2) int32 = the first and the last non-zero word of the row, (words, -1) when there is none.
//   An obs_index outside [0, M) reads no depth: every rendered pixel of the instance is MISSING (the wrapper refuses it on the host).
//   A wave's 64 lanes are 64 consecutive pixels of one instance; every predicate goes through a ballot; the inlier ballot IS the
//   output word, stored by one lane; the counts are popcounts of the ballots, summed per wave in scalars, per workgroup through LDS,
//   and added with one integer atomicAdd per count and workgroup (none for a zero) into counts a fill kernel zeroed; span by integer
//   atomicMin / atomicMax into (words, -1).  Integer sums and extrema do not depend on their order.  A workgroup of four waves takes
//   VF_CHUNK_WORDS consecutive words of one instance; blockIdx.x = chunk N + n, so the workgroups in flight together are the same
//   rows of depth_obs under the instances of a frame (they meet in L2).  8 bytes (9 with masks) read per pixel, one bit written.
//
// SELECTION (verify_select_kernel), one workgroup per frame b; order (K) int32 lists instance indices frame by frame, frame_start
// (B + 1) int64 delimits them (as s6d_vis_owner_from_masks takes them):
//   A claimed bitmap of `words` words starts empty.  The frame's instances are visited in `order`.  For instance n with
//   inl = counts[n][2], beh = counts[n][4]:  fresh = popcount(inlier[n] & ~claimed) -- the lanes stride over span[n], reduce through
//   shuffles and LDS, and every lane takes the same decision from the same integers.  The first status that applies:
//     4  not verifiable   counts[n][0] == 0 (nothing rendered) or flagged[n] != 0 (flagged may be NULL)
//     1                   inl < min_inliers
//     2                   (double)inl < (double)min_fit * (double)(inl + beh)
//     3  explained        (double)fresh < (double)min_fresh * (double)inl
//     0  kept             and only then, after a barrier, inlier[n] is ORed into the bitmap
//   each comparison one double multiply and one compare; the thresholds enter as float.  status (N) int32, fresh (N) int32; an
//   instance `order` does not name keeps the fill kernel's status 4 and fresh 0.  An entry of order outside [0, N) is passed over;
//   an instance named twice is visited twice and keeps the later result (the wrapper refuses both on the host).
//   The bitmap lives in LDS when words <= the limit (VF_LDS_WORDS = 4800 = 480 x 640 / 64, or what s6d_set_verify_lds_words lowered
//   it to), else in the caller's workspace (s6d_verify_select_workspace_bytes: B words 8 bytes): the same code through one pointer,
//   the same results.  No floating-point sum anywhere in either kernel.
#include "s6d_common.h"

#include <math.h>

namespace s6d {

#pragma clang fp contract(off)   // z = depth * unit and d = z - r: one rounding each

typedef unsigned long long u64;

constexpr int VF_THREADS = 256;
constexpr int VF_WAVES = VF_THREADS / kWave;
constexpr int VF_CHUNK_WORDS = 32;                                       // words of one workgroup: eight per wave
constexpr int VF_LDS_WORDS = S6D_VERIFY_LDS_WORDS;                       // 4800: 480 x 640 pixels
constexpr int VF_COUNTS = 8;
static_assert(VF_CHUNK_WORDS % VF_WAVES == 0, "a wave takes every VF_WAVES-th word of the chunk");

int g_s6d_verify_lds_words = 0;                                          // s6d_set_verify_lds_words; 0 = VF_LDS_WORDS

__global__ __launch_bounds__(VF_THREADS) void verify_fill_kernel(int *__restrict__ a, int per, int n, int v0, int v1) {
  const int i = blockIdx.x * VF_THREADS + threadIdx.x;                   // one lane per instance; entry k gets v0 (k even) or v1
  if (i >= n) return;
  for (int k = 0; k < per; ++k) a[(size_t)i * per + k] = (k & 1) ? v1 : v0;
}

__global__ __launch_bounds__(VF_THREADS) void verify_evidence_kernel(const float *__restrict__ render, const float *__restrict__ depth_obs,
                                                                     const int *__restrict__ obs_index, const uint8_t *__restrict__ masks,
                                                                     int N, int M, int plane, int words, float depth_unit, float tau,
                                                                     int *__restrict__ counts, u64 *__restrict__ inlier,
                                                                     int *__restrict__ span) {
  __shared__ int red[VF_COUNTS + 2][VF_WAVES];
  const int chunk = blockIdx.x / N, n = blockIdx.x - chunk * N;          // the instance runs fastest
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int oi = obs_index[n];
  const bool bad = oi < 0 || oi >= M;                                    // the whole workgroup: depth_obs is not read
  const float *R = render + (size_t)n * plane, *Z = depth_obs + (size_t)(bad ? 0 : oi) * plane;
  const uint8_t *D = masks ? masks + (size_t)n * plane : nullptr;
  u64 *I = inlier + (size_t)n * words;
  int cnt[VF_COUNTS] = {0, 0, 0, 0, 0, 0, 0, 0};
  int first = words, last = -1;
  const int j1 = (chunk + 1) * VF_CHUNK_WORDS < words ? (chunk + 1) * VF_CHUNK_WORDS : words;
  for (int j = chunk * VF_CHUNK_WORDS + wave; j < j1; j += VF_WAVES) {   // j is the wave's: the ballots below are of whole waves
    const int p = j * 64 + lane;
    const bool in = p < plane;
    const float r = in ? R[p] : 0.f;
    const float zo = in && !bad ? Z[p] : 0.f;
    const bool det = in && D && D[p] != 0;
    const float z = zo * depth_unit;
    const float d = z - r;
    const bool rendered = r > 0.f;
    const bool measured = z > 0.f && z < INFINITY;
    const bool both = rendered && measured;
    const bool inl = both && fabsf(d) <= tau;
    const u64 b_inl = __ballot(inl);
    cnt[0] += __popcll(__ballot(rendered));
    cnt[1] += __popcll(__ballot(rendered && !measured));
    cnt[2] += __popcll(b_inl);
    cnt[3] += __popcll(__ballot(both && d < -tau));
    cnt[4] += __popcll(__ballot(both && d > tau));
    cnt[5] += __popcll(__ballot(det));
    cnt[6] += __popcll(__ballot(det && rendered));
    cnt[7] += __popcll(__ballot(det && inl));
    if (lane == 0) I[j] = b_inl;                                         // bits of pixels >= plane are zero: `in` failed
    if (b_inl != 0ull) {
      first = j < first ? j : first;
      last = j;
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < VF_COUNTS; ++k) red[k][wave] = cnt[k];
    red[VF_COUNTS][wave] = first;
    red[VF_COUNTS + 1][wave] = last;
  }
  __syncthreads();
  if (threadIdx.x < VF_COUNTS + 2) {
    const int k = threadIdx.x;
    int s = red[k][0];
#pragma unroll
    for (int w = 1; w < VF_WAVES; ++w) {
      const int x = red[k][w];
      s = k < VF_COUNTS ? s + x : k == VF_COUNTS ? (x < s ? x : s) : (x > s ? x : s);
    }
    if (k < VF_COUNTS) {
      if (s != 0) atomicAdd(&counts[(size_t)n * VF_COUNTS + k], s);
    } else if (k == VF_COUNTS) {
      if (s != words) atomicMin(&span[(size_t)n * 2 + 0], s);
    } else {
      if (s != -1) atomicMax(&span[(size_t)n * 2 + 1], s);
    }
  }
}

__global__ __launch_bounds__(VF_THREADS) void verify_select_kernel(const u64 *__restrict__ inlier, const int *__restrict__ counts,
                                                                   const int *__restrict__ span, const int *__restrict__ order,
                                                                   const long *__restrict__ frame_start, const uint8_t *__restrict__ flagged,
                                                                   int N, long K, int words, int use_lds, int min_inliers, float min_fit,
                                                                   float min_fresh, u64 *__restrict__ workspace, int *__restrict__ status,
                                                                   int *__restrict__ fresh_out) {
  __shared__ u64 lds_claimed[VF_LDS_WORDS];
  __shared__ int red[VF_WAVES];
  const int b = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  u64 *claimed = use_lds ? lds_claimed : workspace + (size_t)b * words;  // one code path for both homes of the bitmap
  for (int j = threadIdx.x; j < words; j += VF_THREADS) claimed[j] = 0ull;
  long k0 = frame_start[b], k1 = frame_start[b + 1];                    // clamped to the list: nothing is read outside order (K)
  k0 = k0 < 0 ? 0 : k0;
  k1 = k1 > K ? K : k1;
  __syncthreads();
  for (long k = k0; k < k1; ++k) {
    const int n = order[k];
    if (n < 0 || n >= N) continue;                                       // the whole workgroup
    const int rendered = counts[(size_t)n * VF_COUNTS + 0], inl = counts[(size_t)n * VF_COUNTS + 2], beh = counts[(size_t)n * VF_COUNTS + 4];
    const bool flag = flagged && flagged[n] != 0;
    int lo = span[(size_t)n * 2 + 0], hi = span[(size_t)n * 2 + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > words - 1 ? words - 1 : hi;
    const u64 *I = inlier + (size_t)n * words;
    int c = 0;
    for (int j = lo + threadIdx.x; j <= hi; j += VF_THREADS) c += __popcll(I[j] & ~claimed[j]);
    c = wave_sum_i32(c);
    if (lane == 0) red[wave] = c;
    __syncthreads();                                                     // and every read of the bitmap is done
    int fresh = 0;
#pragma unroll
    for (int w = 0; w < VF_WAVES; ++w) fresh += red[w];
    int st = 0;
    if (rendered == 0 || flag) st = 4;
    else if (inl < min_inliers) st = 1;
    else if ((double)inl < (double)min_fit * (double)(inl + beh)) st = 2;
    else if ((double)fresh < (double)min_fresh * (double)inl) st = 3;
    if (st == 0)
      for (int j = lo + threadIdx.x; j <= hi; j += VF_THREADS) claimed[j] |= I[j];
    if (threadIdx.x == 0) {
      status[n] = st;
      fresh_out[n] = fresh;
    }
    __syncthreads();                                                     // the bitmap and `red` are free for the next instance
  }
}

static inline int verify_lds_limit() { return g_s6d_verify_lds_words > 0 ? g_s6d_verify_lds_words : VF_LDS_WORDS; }

// H W < 2^29 (a pixel index and 64 words stay in an int): S6D_OK and the words of one row, or the refusal
static inline int verify_words(int H, int W, int *words) {
  if (H < 1 || W < 1) return S6D_EINVAL;
  const long plane = (long)H * W;
  if (plane >= (1L << 29)) return S6D_EUNSUPPORTED;
  *words = (int)((plane + 63) / 64);
  return S6D_OK;
}

}  // namespace s6d

using namespace s6d;

extern "C" int s6d_set_verify_lds_words(int words) {
  if (words < 0 || words > VF_LDS_WORDS) return S6D_EINVAL;
  g_s6d_verify_lds_words = words;
  return S6D_OK;
}

extern "C" int s6d_verify_evidence_f32(const float *render, const float *depth_obs, const int32_t *obs_index, const uint8_t *masks, int N,
                                       int M, int H, int W, float depth_unit, float tau, int32_t *counts, uint64_t *inlier, int32_t *span,
                                       void *stream) {
  int words = 0;
  if (N < 0 || M < 1) return S6D_EINVAL;
  const int rc0 = verify_words(H, W, &words);
  if (rc0 != S6D_OK) return rc0;
  if (!(depth_unit > 0.f) || !(depth_unit < INFINITY) || !(tau >= 0.f)) return S6D_EINVAL;
  const long chunks = (words + VF_CHUNK_WORDS - 1) / VF_CHUNK_WORDS;
  if ((long)N * chunks > 0x7fffffffL) return S6D_EUNSUPPORTED;
  if (N == 0) return S6D_OK;
  if (!render || !depth_obs || !obs_index || !counts || !inlier || !span) return S6D_EINVAL;
  hipStream_t s = as_stream(stream);
  const unsigned fill = (unsigned)((N + VF_THREADS - 1) / VF_THREADS);
  hipLaunchKernelGGL(verify_fill_kernel, dim3(fill), dim3(VF_THREADS), 0, s, counts, VF_COUNTS, N, 0, 0);
  int rc = launch_status();
  if (rc != S6D_OK) return rc;
  hipLaunchKernelGGL(verify_fill_kernel, dim3(fill), dim3(VF_THREADS), 0, s, span, 2, N, words, -1);
  rc = launch_status();
  if (rc != S6D_OK) return rc;
  hipLaunchKernelGGL(verify_evidence_kernel, dim3((unsigned)((long)N * chunks)), dim3(VF_THREADS), 0, s, render, depth_obs, obs_index,
                     masks, N, M, H * W, words, depth_unit, tau, counts, reinterpret_cast<u64 *>(inlier), span);
  return launch_status();
}

extern "C" long s6d_verify_select_workspace_bytes(int B, int H, int W) {
  int words = 0;
  if (B < 0 || verify_words(H, W, &words) != S6D_OK) return -1;
  return words <= verify_lds_limit() ? 0L : (long)B * words * 8L;
}

extern "C" int s6d_verify_select(const uint64_t *inlier, const int32_t *counts, const int32_t *span, const int32_t *order,
                                 const long *frame_start, const uint8_t *flagged, int B, int N, long K, int H, int W, int min_inliers,
                                 float min_fit, float min_fresh, void *workspace, int32_t *status, int32_t *fresh, void *stream) {
  int words = 0;
  if (B < 0 || N < 0 || K < 0 || K > N) return S6D_EINVAL;
  const int rc0 = verify_words(H, W, &words);
  if (rc0 != S6D_OK) return rc0;
  if (min_inliers < 0 || !(min_fit >= 0.f) || !(min_fresh >= 0.f)) return S6D_EINVAL;
  if (N == 0) return S6D_OK;
  if (!status || !fresh) return S6D_EINVAL;
  const int use_lds = words <= verify_lds_limit() ? 1 : 0;
  if (B > 0 && (!inlier || !counts || !span || !frame_start || (K > 0 && !order) || (!use_lds && !workspace))) return S6D_EINVAL;
  hipStream_t s = as_stream(stream);
  const unsigned fill = (unsigned)((N + VF_THREADS - 1) / VF_THREADS);
  hipLaunchKernelGGL(verify_fill_kernel, dim3(fill), dim3(VF_THREADS), 0, s, status, 1, N, 4, 4);
  int rc = launch_status();
  if (rc != S6D_OK) return rc;
  hipLaunchKernelGGL(verify_fill_kernel, dim3(fill), dim3(VF_THREADS), 0, s, fresh, 1, N, 0, 0);
  rc = launch_status();
  if (rc != S6D_OK || B == 0) return rc;
  hipLaunchKernelGGL(verify_select_kernel, dim3((unsigned)B), dim3(VF_THREADS), 0, s, reinterpret_cast<const u64 *>(inlier), counts, span,
                     order, frame_start, flagged, N, K, words, use_lds, min_inliers, min_fit, min_fresh,
                     reinterpret_cast<u64 *>(workspace), status, fresh);
  return launch_status();
}
