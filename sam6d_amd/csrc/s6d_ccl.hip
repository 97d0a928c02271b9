// Connected components of binary masks and SAM's small-region clean-up on the device (gfx950).  The quantities are DEFINED in
// include/sam6d_hip.h (s6d_remove_small_regions_u8) and DESIGN section 13, operation by operation; tests/small_regions_ref.py restates
// them in plain loops and every comparison with it is `equal`.  cv2 is not part of this project and nothing claims equality with it.
//
// A pixel is FOREGROUND when (byte != 0) != background.  Connectivity is 8.  The label of a foreground pixel is the row-major index
// (y W + x, inside its own mask) of the first pixel of its component, i.e. the component's minimum index; -1 elsewhere.
//
// Labels form a union-find forest in an int32 plane L: L[p] <= p, L[p] is a pixel of p's component, a root has L[p] = p.  A link is
// only ever made from a root to a smaller index of the other set (atomicMin), so the root of a set is its minimum: the canonical label.
//
//   uf_find    follows L from a to a root.  TERMINATES: every step goes to a strictly smaller index, bounded below by 0.  A value that
//              is stale (another lane linked the pixel meanwhile, or a cache still holds the old line) is still a pixel of the same
//              set with an index <= the pixel's, so a stale read costs steps, never correctness; the reads are volatile so that each
//              one is a load.  (uf_find_static: the same walk with plain loads, for the kernels in which no lane changes L.)
//   uf_union   a = find(a), b = find(b); equal: done; else link the larger (a) below the smaller with old = atomicMin(&L[a], b).
//              old == a: a was a root and now points at b, done.  Otherwise another lane had linked a to old < a first; L[a] is now
//              min(old, b), both in the merged set, and what is left is union(old, b): go round with a = old.  TERMINATES: a round that
//              does not return replaces max(a, b) by a strictly smaller index and never raises the other, so a + b falls every round
//              and is bounded below by 0 (labels only decrease).  Nothing waits for another lane, wave or workgroup: there is no spin
//              on a value somebody else must write, and kernel boundaries are the only grid-wide ordering.
//
// ccl_tile_kernel<BG>   one workgroup per (mask, tile of S6D_CCL_TILE_H x S6D_CCL_TILE_W), four pixels per lane (a wave instruction = one
//                       tile row).  Forest of the tile in LDS: each foreground pixel is united with the neighbours of the decision tree
//                       "N, else (W, else NW) and NE" inside the tile (a skipped neighbour is joined to a taken one by that pixel's own
//                       step).  After the barrier every pixel finds its local root; the pixels of a wave that share a root are counted
//                       with ballots and ONE LDS atomicAdd per distinct root and wave.  Written: L[p] = global index of the local root
//                       (-1 on background), A[p] = pixels of the local component at its local root, 0 elsewhere.
// ccl_seam_kernel       one lane per pixel of a tile's first row (tile rows >= 1): united with (y-1, x), else with (y-1, x-1) and
//                       (y-1, x+1); and per pixel of a tile's first column (tile columns >= 1): united with (y, x-1), else with
//                       (y-1, x-1) and (y+1, x-1).  Two 8-adjacent pixels of different tiles differ in the tile row (then one lies on
//                       a first row, the other right above it, |dx| <= 1, corners included) or only in the tile column (then one lies on
//                       a first column, the other left of it, |dy| <= 1): every such pair is united here or joined through a pair that
//                       is.  Global atomicMin union-find on L.
// ccl_area_kernel       a local root p (A[p] > 0) that is not its component's root r adds A[p] to A[r]: one integer atomic per
//                       (component, tile) -- the per-pixel sums were already folded per wave and tile in LDS.  Roots only receive and
//                       non-roots only give, so no value is read while it changes.  After the kernel A[r] is the component's area.
// ccl_flatten_kernel    L[p] = find(p).  With `best`: per mask atomicMax of (area << 32) | ~root over the roots, the maximum of a wave
//                       first (shuffles), one atomic per wave -- the largest area, and among equal areas the smallest root.
// ccl_apply_kernel<BG>  BG (holes): a background pixel of a component with area < min_area is set; flag bit 0 when there is one.
//                       !BG (islands, in place on the result of the holes step): a set pixel of a small component raises flag bit 1;
//                       it stays set when its component is not small, or, if the best area of the mask is small too (every component
//                       is small), when its root is the best one.  Box of the result: min / max of x and y over a wave's set pixels
//                       (shuffles), then four integer atomics per wave that has any.
// ccl_init_kernel / ccl_finish_kernel   per-mask state: best = 0, flags = 0, box = (W, H, -1, -1) -> changed = flags != 0 and the box,
//                       (0, 0, 0, 0) for an empty mask.
// Every quantity is an integer and every atomic an integer min / max / add / or: results do not depend on scheduling, N or chunking.
#include "s6d_common.h"

namespace s6d {

typedef unsigned long long u64;

constexpr int CCL_TH = S6D_CCL_TILE_H, CCL_TW = S6D_CCL_TILE_W;
constexpr int CCL_THREADS = 256;
constexpr int CCL_TILE = CCL_TH * CCL_TW;
constexpr int CCL_PPL = CCL_TILE / CCL_THREADS;                          // pixels of a lane in the tile kernel
static_assert(CCL_TW == kWave && CCL_TILE % CCL_THREADS == 0, "a wave instruction of the tile kernel is one tile row");

__device__ __forceinline__ int uf_find(const int *L, int a) {
  for (;;) {
    const int p = *reinterpret_cast<const volatile int *>(L + a);
    if (p == a) return a;
    a = p;
  }
}

// the same walk through a forest that no lane changes during the kernel: plain (cacheable) loads
__device__ __forceinline__ int uf_find_static(const int *__restrict__ L, int a) {
  for (;;) {
    const int p = L[a];
    if (p == a) return a;
    a = p;
  }
}

__device__ __forceinline__ void uf_union(int *L, int a, int b) {
  for (;;) {
    a = uf_find(L, a);
    b = uf_find(L, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(&L[a], b);
    if (old == a) return;
    a = old;
  }
}

// count[key] += the number of lanes of the wave with this key, one atomicAdd per distinct key (every lane of the wave calls this)
__device__ __forceinline__ void wave_count_by_key(int *count, int key, bool valid) {
  const int lane = lane_id();
  bool pending = valid;
  for (;;) {
    const u64 open = __ballot(pending);
    if (open == 0) break;
    const int lead = __ffsll(open) - 1;
    const int k0 = __shfl(key, lead);
    const bool same = pending && key == k0;
    const u64 m = __ballot(same);
    if (lane == lead) atomicAdd(&count[k0], __popcll(m));
    pending = pending && !same;
  }
}

template <bool BG>
__global__ __launch_bounds__(CCL_THREADS) void ccl_tile_kernel(const uint8_t *__restrict__ masks, int H, int W, int tiles_x,
                                                               int tiles, int *__restrict__ labels, int *__restrict__ areas) {
  __shared__ int L[CCL_TILE];
  __shared__ int C[CCL_TILE];
  const int n = blockIdx.x / tiles, tile = blockIdx.x - n * tiles;
  const int ty0 = (tile / tiles_x) * CCL_TH, tx0 = (tile % tiles_x) * CCL_TW;
  const size_t base = (size_t)n * H * W;
  const int lx = threadIdx.x & (CCL_TW - 1), x = tx0 + lx;
  bool fg[CCL_PPL];
#pragma unroll
  for (int k = 0; k < CCL_PPL; ++k) {
    const int p = threadIdx.x + k * CCL_THREADS, y = ty0 + p / CCL_TW;
    fg[k] = y < H && x < W && ((masks[base + (size_t)y * W + x] != 0) != BG);
    L[p] = fg[k] ? p : -1;
    C[p] = 0;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < CCL_PPL; ++k) {
    const int p = threadIdx.x + k * CCL_THREADS;
    if (!fg[k]) continue;
    const bool up = p >= CCL_TW, left = lx > 0, right = lx < CCL_TW - 1;
    if (up && L[p - CCL_TW] >= 0) {
      uf_union(L, p, p - CCL_TW);
    } else {
      if (left && L[p - 1] >= 0) uf_union(L, p, p - 1);
      else if (up && left && L[p - CCL_TW - 1] >= 0) uf_union(L, p, p - CCL_TW - 1);
      if (up && right && L[p - CCL_TW + 1] >= 0) uf_union(L, p, p - CCL_TW + 1);
    }
  }
  __syncthreads();
  int root[CCL_PPL];
#pragma unroll
  for (int k = 0; k < CCL_PPL; ++k) {
    root[k] = fg[k] ? uf_find(L, threadIdx.x + k * CCL_THREADS) : -1;
    wave_count_by_key(C, root[k], fg[k]);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < CCL_PPL; ++k) {
    const int p = threadIdx.x + k * CCL_THREADS, y = ty0 + p / CCL_TW;
    if (y >= H || x >= W) continue;
    const size_t o = base + (size_t)y * W + x;
    labels[o] = fg[k] ? (ty0 + root[k] / CCL_TW) * W + tx0 + root[k] % CCL_TW : -1;
    areas[o] = root[k] == p ? C[p] : 0;
  }
}

__global__ __launch_bounds__(CCL_THREADS) void ccl_seam_kernel(int H, int W, int row_items, int items, int blocks, int *labels) {
  const int n = blockIdx.x / blocks;
  const int i = (blockIdx.x - n * blocks) * CCL_THREADS + threadIdx.x;
  if (i >= items) return;
  int *L = labels + (size_t)n * H * W;
  const volatile int *V = L;
  if (i < row_items) {
    const int y = (i / W + 1) * CCL_TH, x = i - (i / W) * W;
    const int p = y * W + x, q = p - W;
    if (V[p] < 0) return;
    if (V[q] >= 0) {
      uf_union(L, p, q);
    } else {
      if (x > 0 && V[q - 1] >= 0) uf_union(L, p, q - 1);
      if (x < W - 1 && V[q + 1] >= 0) uf_union(L, p, q + 1);
    }
  } else {
    const int j = i - row_items;
    const int x = (j / H + 1) * CCL_TW, y = j - (j / H) * H;
    const int p = y * W + x, q = p - 1;
    if (V[p] < 0) return;
    if (V[q] >= 0) {
      uf_union(L, p, q);
    } else {
      if (y > 0 && V[q - W] >= 0) uf_union(L, p, q - W);
      if (y < H - 1 && V[q + W] >= 0) uf_union(L, p, q + W);
    }
  }
}

__global__ __launch_bounds__(CCL_THREADS) void ccl_area_kernel(int HW, int blocks, const int *__restrict__ labels,
                                                               int *__restrict__ areas) {
  const int n = blockIdx.x / blocks;
  const int p = (blockIdx.x - n * blocks) * CCL_THREADS + threadIdx.x;
  if (p >= HW) return;
  const int *L = labels + (size_t)n * HW;
  int *A = areas + (size_t)n * HW;
  const int a = A[p];
  if (a <= 0) return;
  const int r = uf_find_static(L, p);
  if (r != p) atomicAdd(&A[r], a);
}

__global__ __launch_bounds__(CCL_THREADS) void ccl_flatten_kernel(int HW, int blocks, int *labels,
                                                                  const int *__restrict__ areas, u64 *__restrict__ best) {
  const int n = blockIdx.x / blocks;
  const int p = (blockIdx.x - n * blocks) * CCL_THREADS + threadIdx.x;
  int *L = labels + (size_t)n * HW;
  u64 key = 0;
  if (p < HW && L[p] >= 0) {
    const int r = uf_find(L, p);
    L[p] = r;
    if (best != nullptr && r == p) key = ((u64)(unsigned)areas[(size_t)n * HW + p] << 32) | (unsigned)~p;
  }
  if (best == nullptr) return;                                           // (the whole grid)
  key = wave_max_u64(key);
  if (lane_id() == 0 && key != 0) atomicMax(&best[n], key);
}

template <bool BG>
__global__ __launch_bounds__(CCL_THREADS) void ccl_apply_kernel(const uint8_t *masks, int H, int W, int blocks,
                                                                long min_area, const int *__restrict__ labels,
                                                                const int *__restrict__ areas, const u64 *__restrict__ best,
                                                                uint8_t *out, int *__restrict__ flags,
                                                                int *__restrict__ box) {
  const int n = blockIdx.x / blocks, HW = H * W;
  const int p = (blockIdx.x - n * blocks) * CCL_THREADS + threadIdx.x;
  const size_t base = (size_t)n * HW;
  const bool valid = p < HW;
  const bool set = valid && masks[base + p] != 0;
  bool small = false, keep = set;
  if (valid && set != BG) {
    const int r = uf_find_static(labels + base, p);                      // (islands: flattened, one step)
    small = (long)areas[base + r] < min_area;
    if (BG) {
      keep = small;
    } else {
      const u64 b = best[n];
      keep = (long)(b >> 32) >= min_area ? !small : r == (int)~(unsigned)b;
    }
  }
  if (valid) out[base + p] = keep ? 1 : 0;
  if (__ballot(small) != 0 && lane_id() == 0) atomicOr(&flags[n], BG ? 1 : 2);
  if (BG) return;
  if (__ballot(keep) == 0) return;                                       // (the whole wave)
  const int y = valid ? p / W : 0, x = valid ? p - y * W : 0;
  int x0 = keep ? x : W, y0 = keep ? y : H, x1 = keep ? x : -1, y1 = keep ? y : -1;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int a = __shfl_xor(x0, o), b = __shfl_xor(y0, o), c = __shfl_xor(x1, o), d = __shfl_xor(y1, o);
    x0 = a < x0 ? a : x0;
    y0 = b < y0 ? b : y0;
    x1 = c > x1 ? c : x1;
    y1 = d > y1 ? d : y1;
  }
  if (lane_id() == 0) {
    atomicMin(&box[4 * n], x0);
    atomicMin(&box[4 * n + 1], y0);
    atomicMax(&box[4 * n + 2], x1);
    atomicMax(&box[4 * n + 3], y1);
  }
}

__global__ __launch_bounds__(CCL_THREADS) void ccl_init_kernel(int N, int H, int W, u64 *__restrict__ best, int *__restrict__ flags,
                                                               int *__restrict__ box) {
  const int n = blockIdx.x * CCL_THREADS + threadIdx.x;
  if (n >= N) return;
  best[n] = 0;
  flags[n] = 0;
  box[4 * n] = W;
  box[4 * n + 1] = H;
  box[4 * n + 2] = -1;
  box[4 * n + 3] = -1;
}

__global__ __launch_bounds__(CCL_THREADS) void ccl_finish_kernel(int N, const int *__restrict__ flags, const int *__restrict__ box,
                                                                 uint8_t *__restrict__ changed, int *__restrict__ boxes) {
  const int n = blockIdx.x * CCL_THREADS + threadIdx.x;
  if (n >= N) return;
  changed[n] = flags[n] != 0 ? 1 : 0;
  const bool empty = box[4 * n + 2] < 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) boxes[4 * n + k] = empty ? 0 : box[4 * n + k];
}

struct CclPlan {
  int tiles_x, tiles, row_items, items, seam_blocks, pix_blocks;
  long plane;                                                            // bytes of one (N, H, W) int32 plane
};

// sizes -> plan, or an error code: every grid is one-dimensional and must fit 2^31 - 1 workgroups
static int ccl_plan(int N, int H, int W, CclPlan *pl) {
  if (N < 0 || H < 1 || W < 1) return S6D_EINVAL;
  const long HW = (long)H * W;
  if (HW > 0x7fffffffL) return S6D_EINVAL;
  if (HW > 0x7fffffffL - CCL_THREADS) return S6D_EUNSUPPORTED;             // (a pixel index past the last workgroup's end stays an int)
  const long tiles_y = (H + CCL_TH - 1) / CCL_TH, tiles_x = (W + CCL_TW - 1) / CCL_TW;
  const long row_items = (tiles_y - 1) * W, items = row_items + (tiles_x - 1) * H;
  const long seam_blocks = (items + CCL_THREADS - 1) / CCL_THREADS, pix_blocks = (HW + CCL_THREADS - 1) / CCL_THREADS;
  if (N * tiles_y * tiles_x > 0x7fffffffL || N * pix_blocks > 0x7fffffffL) return S6D_EUNSUPPORTED;
  pl->tiles_x = (int)tiles_x;
  pl->tiles = (int)(tiles_y * tiles_x);
  pl->row_items = (int)row_items;
  pl->items = (int)items;
  pl->seam_blocks = (int)seam_blocks;
  pl->pix_blocks = (int)pix_blocks;
  pl->plane = (long)N * HW * 4;
  return S6D_OK;
}

// the forest of one polarity: tile, seam; with `areas_too` the component areas at the roots
template <bool BG>
static int ccl_label(const uint8_t *masks, int N, int H, int W, const CclPlan &pl, int *labels, int *areas, bool areas_too,
                     hipStream_t s) {
  hipLaunchKernelGGL(ccl_tile_kernel<BG>, dim3((unsigned)((long)N * pl.tiles)), dim3(CCL_THREADS), 0, s, masks, H, W, pl.tiles_x,
                     pl.tiles, labels, areas);
  if (pl.items > 0)
    hipLaunchKernelGGL(ccl_seam_kernel, dim3((unsigned)((long)N * pl.seam_blocks)), dim3(CCL_THREADS), 0, s, H, W, pl.row_items,
                       pl.items, pl.seam_blocks, labels);
  if (areas_too)
    hipLaunchKernelGGL(ccl_area_kernel, dim3((unsigned)((long)N * pl.pix_blocks)), dim3(CCL_THREADS), 0, s, H * W, pl.pix_blocks, labels,
                       areas);
  return launch_status();
}

}  // namespace s6d

using namespace s6d;

extern "C" long s6d_small_regions_workspace_bytes(int N, int H, int W) {
  CclPlan pl;
  if (ccl_plan(N, H, W, &pl) != S6D_OK) return -1;
  return 2 * pl.plane + (long)N * (8 + 4 + 16) + 8;
}

extern "C" int s6d_label_components_u8(const uint8_t *masks, int N, int H, int W, int background, void *workspace, int32_t *labels,
                                       void *stream) {
  CclPlan pl;
  int rc = ccl_plan(N, H, W, &pl);
  if (rc != S6D_OK) return rc;
  if (background != 0 && background != 1) return S6D_EINVAL;
  if (N == 0) return S6D_OK;
  if (!masks || !workspace || !labels) return S6D_EINVAL;
  hipStream_t s = as_stream(stream);
  int *areas = reinterpret_cast<int *>(workspace);
  rc = background ? ccl_label<true>(masks, N, H, W, pl, labels, areas, false, s)
                  : ccl_label<false>(masks, N, H, W, pl, labels, areas, false, s);
  if (rc != S6D_OK) return rc;
  hipLaunchKernelGGL(ccl_flatten_kernel, dim3((unsigned)((long)N * pl.pix_blocks)), dim3(CCL_THREADS), 0, s, H * W, pl.pix_blocks, labels,
                     areas, (u64 *)nullptr);
  return launch_status();
}

extern "C" int s6d_remove_small_regions_u8(const uint8_t *masks, int N, int H, int W, long min_area, void *workspace, uint8_t *out,
                                           uint8_t *changed, int32_t *boxes, void *stream) {
  CclPlan pl;
  int rc = ccl_plan(N, H, W, &pl);
  if (rc != S6D_OK) return rc;
  if (min_area < 1) return S6D_EINVAL;
  if (N == 0) return S6D_OK;
  if (!masks || !workspace || !out || !changed || !boxes) return S6D_EINVAL;
  hipStream_t s = as_stream(stream);
  char *ws = reinterpret_cast<char *>(workspace);
  int *labels = reinterpret_cast<int *>(ws), *areas = reinterpret_cast<int *>(ws + pl.plane);
  u64 *best = reinterpret_cast<u64 *>(ws + 2 * pl.plane);
  int *flags = reinterpret_cast<int *>(best + N), *box = flags + N;
  const dim3 per_mask((unsigned)((N + CCL_THREADS - 1) / CCL_THREADS)), per_pixel((unsigned)((long)N * pl.pix_blocks));
  hipLaunchKernelGGL(ccl_init_kernel, per_mask, dim3(CCL_THREADS), 0, s, N, H, W, best, flags, box);
  rc = ccl_label<true>(masks, N, H, W, pl, labels, areas, true, s);                                     // holes
  if (rc != S6D_OK) return rc;
  hipLaunchKernelGGL(ccl_apply_kernel<true>, per_pixel, dim3(CCL_THREADS), 0, s, masks, H, W, pl.pix_blocks, min_area, labels, areas,
                     best, out, flags, box);
  rc = ccl_label<false>(out, N, H, W, pl, labels, areas, true, s);                                      // islands, on that result
  if (rc != S6D_OK) return rc;
  hipLaunchKernelGGL(ccl_flatten_kernel, per_pixel, dim3(CCL_THREADS), 0, s, H * W, pl.pix_blocks, labels, areas, best);
  hipLaunchKernelGGL(ccl_apply_kernel<false>, per_pixel, dim3(CCL_THREADS), 0, s, out, H, W, pl.pix_blocks, min_area, labels, areas, best,
                     out, flags, box);
  hipLaunchKernelGGL(ccl_finish_kernel, per_mask, dim3(CCL_THREADS), 0, s, N, flags, box, changed, boxes);
  return launch_status();
}
