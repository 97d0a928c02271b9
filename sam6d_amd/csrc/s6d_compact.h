// What a workgroup of the PEM pre-processing (s6d_pempre.hip) and of the template onboarding (s6d_onboard.hip) does with the pixels
// of one mask, written once for both: the count and extent reduction behind the reference's get_bbox, the in-order compaction
// (wave ballot ranks + a 16-entry wave prefix), and the walk of a square crop that compacts the pixels a caller keeps.
#pragma once
#include "s6d_common.h"
#include "s6d_crop_params.h"

namespace s6d {

constexpr int kCmpThreads = 1024;

// Extent of a pixel set as [-ymin, ymax, -xmin, xmax]: the minima are kept negated, so that one max-reduction serves all four.
__device__ __forceinline__ void extent_init(int *b, int H, int W) {
  b[0] = -H;
  b[1] = -1;
  b[2] = -W;
  b[3] = -1;
}

__device__ __forceinline__ void extent_add(int *b, int y, int x) {
  b[0] = max(b[0], -y);
  b[1] = max(b[1], y);
  b[2] = max(b[2], -x);
  b[3] = max(b[3], x);
}

// Sums cnt and folds the extents of SETS pixel sets (b[4 * s ..] is set s) over the workgroup: wave butterfly, one LDS entry per wave,
// serial fold on thread 0, which alone gets the totals (b in place, the count returned).  Integers throughout: exact in any order.
template <int SETS>
__device__ __forceinline__ long block_extents(int cnt, int (&b)[4 * SETS]) {
  constexpr int kWaves = kCmpThreads / 64;
  __shared__ int s_cnt[kWaves], s_b[4 * SETS][kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cnt += __shfl_xor(cnt, o);
#pragma unroll
    for (int k = 0; k < 4 * SETS; ++k) b[k] = max(b[k], __shfl_xor(b[k], o));
  }
  if (lane == 0) {
    s_cnt[wave] = cnt;
#pragma unroll
    for (int k = 0; k < 4 * SETS; ++k) s_b[k][wave] = b[k];
  }
  __syncthreads();
  long c = 0;
  if (tid == 0) {
    for (int w = 0; w < kWaves; ++w) {
      c += s_cnt[w];
      for (int k = 0; k < 4 * SETS; ++k) b[k] = max(b[k], s_b[k][w]);
    }
  }
  return c;
}

// box = get_bbox (square_box) of the set whose reduced extent is b, or of the whole view where the caller found no set
__device__ __forceinline__ void extent_box(bool found, const int *b, int H, int W, long *box) {
  square_box(found ? -b[0] : 0, found ? b[1] + 1 : H, found ? -b[2] : 0, found ? b[3] + 1 : W, H, W, box);
}

// in-order compaction step of one 1024-element chunk: returns this lane's output position (or -1) and advances *base
__device__ __forceinline__ long block_rank(bool keep, long *base, unsigned *wave_tot) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long bal = __ballot(keep);
  const int rank = __popcll(bal & ((1ull << lane) - 1ull));
  if (lane == 0) wave_tot[wave] = (unsigned)__popcll(bal);
  __syncthreads();
  long off = *base;
  unsigned tot = 0;
  for (int w = 0; w < kCmpThreads / 64; ++w) {
    if (w < wave) off += wave_tot[w];
    tot += wave_tot[w];
  }
  __syncthreads();                                      // everyone has read base / wave_tot before they change
  if (tid == 0) *base += tot;
  return keep ? off + rank : -1;
}

// "mask -> choose" of the reference over one square crop: the workgroup walks box = [y1,y2,x1,x2] of an H x W view in row-major crop
// order, 1024 pixels a chunk; keep(pix) says whether the pixel at flat view index pix stays, emit(slot, j, y, x) stores crop pixel j
// = view pixel (y, x) at its rank.  *n_out = how many stayed.  Nothing is read or written, and *n_out = 0, where `on` is false, the
// box does not lie inside the view, or its area exceeds cap, the caller's slots per item.
template <class Keep, class Emit>
__device__ __forceinline__ void compact_crop(const long *box, bool on, int H, int W, long cap, long *n_out, Keep keep, Emit emit) {
  __shared__ unsigned wave_tot[kCmpThreads / 64];
  __shared__ long base;
  const int tid = threadIdx.x;
  if (tid == 0) base = 0;
  __syncthreads();
  const long y1 = box[0], y2 = box[1], x1 = box[2], x2 = box[3];
  if (on && y1 >= 0 && y1 <= y2 && y2 <= H && x1 >= 0 && x1 <= x2 && x2 <= W && (y2 - y1) * (x2 - x1) <= cap) {
    const int bw = (int)(x2 - x1), area = (int)(y2 - y1) * bw;    // a crop is at most H * W < 2^31 pixels: 32-bit index arithmetic
    for (int c0 = 0; c0 < area; c0 += kCmpThreads) {
      const int j = c0 + tid;
      bool k = false;
      int y = 0, x = 0;
      if (j < area) {
        const int r = j / bw;
        y = (int)y1 + r;
        x = (int)x1 + (j - r * bw);
        k = keep(y * W + x);
      }
      const long pos = block_rank(k, &base, wave_tot);
      if (k) emit(pos, j, y, x);
    }
  }
  __syncthreads();
  if (tid == 0) *n_out = base;
}

}  // namespace s6d
