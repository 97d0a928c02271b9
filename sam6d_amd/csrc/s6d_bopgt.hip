// BOP ground-truth derivation on the device (gfx950): from ONE rendered depth canvas per annotated instance (s6d_raster_depth_f32,
// csrc/s6d_raster.hip) and the measured depth image, the instance's mask, its visible mask, their pixel counts and inclusive
// extents; and the diameter of a model.  bop_toolkit is not part of this project and none of its text is used: the quantities are
// DEFINED here, operation by operation, and the tests pin the kernels to an independent restatement of this header
// (tests/bopgt_ref.py).  Nothing claims equality with the toolkit's files.
//
// Fixed arithmetic (float32, every operation rounded on its own: contraction is off, `/` and sqrtf are the correctly rounded forms).
//
// gt_visibility_kernel  workgroups of 256 lanes, each over a run of GT_CHUNK canvas pixels of ONE instance n.  canvas[n] is
//                   (H + 2 my, W + 2 mx): camera Z of the instance rendered with cx + mx, cy + my, 0 on background.  Image pixel
//                   (u, v) is canvas pixel (u + mx, v + my); everything about the image is read from that window of the one
//                   canvas, so visib <= mask <= all holds by construction.  Zt = depth_test[test_index[n]] at (u, v), 0 = missing;
//                   fx fy cx cy = cams[n], the IMAGE's camera.
//   all        Zg > 0, anywhere on the canvas.
//   window     0 <= u < W && 0 <= v < H; there  mask = all,  r = sqrtf((a a + b b) + 1) with a = ((float)u - cx) / fx,
//              b = ((float)v - cy) / fy,  Dg = Zg r,  Dt = Zt r,  valid = mask && Zt > 0,
//              visib = mask && ((Dg - Dt) <= delta || Zt == 0)  -- vis_gt of vsd_counts_kernel, the same device function
//              (csrc/s6d_bopvis.h).
//   outputs    mask, mask_visib (N,H,W) uint8 0 / 1, every pixel written;  counts (N,4) = all, in-image, valid, visib;
//              extents (N,2,4) = xmin ymin xmax ymax (maximum inclusive) of `all` (row 0) and of `visib` (row 1) in IMAGE
//              coordinates (canvas minus the margin: negative or >= W / H outside the frame).
//   reduction  integer counters and extents per lane, the wave (shuffles), the four waves (LDS), then one integer atomicAdd /
//              atomicMin / atomicMax per output and workgroup, none from a workgroup that saw nothing, into outputs a fill kernel
//              preset to 0 and to INT_MAX INT_MAX INT_MIN INT_MIN (= empty).  Integer sums and extrema do not depend on their
//              order: an instance has the same result alone, in a batch and under any chunking.
//              A test_index outside [0, M) leaves the instance's counts and extents at the preset and its masks zero (the wrapper
//              refuses it on the host).
//
// model_diameter_kernel  the maximum over all vertex pairs of  d2 = (dx dx + dy dy) + dz dz,  dx = xi - xj ...; ONE sqrtf of the
//                   maximum (sqrtf is monotone: the bits of the maximum of the roots).  A d2 that is not finite counts as +inf.
//   tiles      vertices in tiles of 256; the tile pairs (ti <= tj) are the steps of PERSISTENT workgroups (step k of the ntiles^2
//              grid, k = blockIdx.x, += gridDim.x; a step with tj < ti returns at once): one workgroup per pair would end in one
//              atomic per pair on ONE address -- 1.9 10^6 of them at V = 5 10^5 -- where a persistent workgroup keeps its maximum
//              in registers and issues one.  The tj tile sits in LDS as (x, y, z, -) and every lane reads the same address (a
//              broadcast, no bank conflict); each lane keeps its own vertex of ti in registers.  A tile's tail repeats the last
//              vertex, which adds only pairs that exist.
//   maximum    taken on the BITS as unsigned integers: d2 is never negative, so for finite values and +inf that is the float
//              order, and every NaN pattern lies above +inf's; the workgroup clamps its maximum to +inf's bits.  Wave (shuffles),
//              LDS, one atomicMax per workgroup into a zeroed word; a last kernel of one lane takes the sqrtf.  No (V, V) buffer,
//              and the workspace is that one word whatever V is.
#include "s6d_bopvis.h"

#include <limits.h>

namespace s6d {

#pragma clang fp contract(off)   // the stated float32 operations, one rounding each

constexpr int GT_THREADS = 256;
constexpr int GT_WAVES = GT_THREADS / kWave;
constexpr int GT_CHUNK = GT_THREADS * 8;                                 // canvas pixels of one workgroup
constexpr int GT_TERMS = 12;                                             // 4 counts, 2 x (xmin ymin | xmax ymax)
constexpr unsigned GT_INF_BITS = 0x7f800000u;
constexpr int MD_TILE = 256;
constexpr int MD_GRID = 256 * 8;                                         // persistent: eight workgroups of four waves per CU

__global__ __launch_bounds__(GT_THREADS) void gt_fill_kernel(int *__restrict__ counts, int *__restrict__ extents, int n) {
  const int i = blockIdx.x * GT_THREADS + threadIdx.x;                   // one lane per instance
  if (i >= n) return;
#pragma unroll
  for (int k = 0; k < 4; ++k) counts[(size_t)i * 4 + k] = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) extents[(size_t)i * 8 + k] = (k & 2) ? INT_MIN : INT_MAX;
}

__device__ __forceinline__ int wave_min_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int w = __shfl_xor(v, o);
    v = w < v ? w : v;
  }
  return v;
}
__device__ __forceinline__ int wave_max_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int w = __shfl_xor(v, o);
    v = w > v ? w : v;
  }
  return v;
}

__global__ __launch_bounds__(GT_THREADS) void gt_visibility_kernel(const float *__restrict__ canvas, const float *__restrict__ depth_test,
                                                                   const int *__restrict__ test_index, const float *__restrict__ cams,
                                                                   int M, int H, int W, int mx, int my, long cplane, int chunks,
                                                                   float delta, uint8_t *__restrict__ mask,
                                                                   uint8_t *__restrict__ mask_visib, int *__restrict__ counts,
                                                                   int *__restrict__ extents) {
  __shared__ int red[GT_TERMS][GT_WAVES];
  const int n = blockIdx.x / chunks, chunk = blockIdx.x - n * chunks;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ti = test_index[n];
  const bool bad = ti < 0 || ti >= M;                                    // the whole workgroup: depth_test is not read, the masks are zeroed
  const float fx = cams[(size_t)n * 4 + 0], fy = cams[(size_t)n * 4 + 1], cx = cams[(size_t)n * 4 + 2], cy = cams[(size_t)n * 4 + 3];
  const long plane = (long)H * W;
  const int Wc = W + 2 * mx;
  const float *ZG = canvas + (size_t)n * cplane, *ZT = depth_test + (size_t)(bad ? 0 : ti) * plane;
  uint8_t *MK = mask + (size_t)n * plane, *MV = mask_visib + (size_t)n * plane;
  int cnt[4] = {0, 0, 0, 0};
  int lo[4] = {INT_MAX, INT_MAX, INT_MAX, INT_MAX}, hi[4] = {INT_MIN, INT_MIN, INT_MIN, INT_MIN};          // x y of all, x y of visib
  const long p0 = (long)chunk * GT_CHUNK, p1 = p0 + GT_CHUNK < cplane ? p0 + GT_CHUNK : cplane;
  // the canvas row and column of this lane's first pixel by one division, of its next ones by a step of GT_THREADS pixels
  long p = p0 + threadIdx.x;
  int vc = (int)(p / Wc), uc = (int)(p - (long)vc * Wc);
  const int step_v = GT_THREADS / Wc, step_u = GT_THREADS - step_v * Wc;
  for (; p < p1; p += GT_THREADS) {
    const int u = uc - mx, v = vc - my;
    const float zg = ZG[p];
    const bool all = !bad && zg > 0.f;
    if (all) {
      cnt[0] += 1;
      lo[0] = u < lo[0] ? u : lo[0];
      lo[1] = v < lo[1] ? v : lo[1];
      hi[0] = u > hi[0] ? u : hi[0];
      hi[1] = v > hi[1] ? v : hi[1];
    }
    if (u >= 0 && u < W && v >= 0 && v < H) {
      const long q = (long)v * W + u;
      bool visib = false;
      if (all) {
        const float zt = ZT[q];
        const float r = bop_ray_factor(u, v, fx, fy, cx, cy);
        const float Dg = zg * r, Dt = zt * r;
        visib = bop_visible(zg, zt, Dg, Dt, delta);
        cnt[1] += 1;
        cnt[2] += zt > 0.f ? 1 : 0;
        if (visib) {
          cnt[3] += 1;
          lo[2] = u < lo[2] ? u : lo[2];
          lo[3] = v < lo[3] ? v : lo[3];
          hi[2] = u > hi[2] ? u : hi[2];
          hi[3] = v > hi[3] ? v : hi[3];
        }
      }
      MK[q] = all ? 1 : 0;
      MV[q] = visib ? 1 : 0;
    }
    uc += step_u;
    vc += step_v;
    if (uc >= Wc) {
      uc -= Wc;
      vc += 1;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int s = wave_sum_i32(cnt[k]), a = wave_min_i32(lo[k]), b = wave_max_i32(hi[k]);
    if (lane == 0) {
      red[k][wave] = s;
      red[4 + k][wave] = a;
      red[8 + k][wave] = b;
    }
  }
  __syncthreads();
  if (threadIdx.x < GT_TERMS) {
    const int k = threadIdx.x;
    int s = red[k][0];
#pragma unroll
    for (int w = 1; w < GT_WAVES; ++w) {
      const int x = red[k][w];
      s = k < 4 ? s + x : k < 8 ? (x < s ? x : s) : (x > s ? x : s);
    }
    // extents (n, row, 4): row 0 = all, row 1 = visib; lo[0..1] / hi[0..1] belong to row 0, lo[2..3] / hi[2..3] to row 1
    if (k < 4) {
      if (s != 0) atomicAdd(&counts[(size_t)n * 4 + k], s);
    } else if (k < 8) {
      const int j = k - 4;
      if (s != INT_MAX) atomicMin(&extents[(size_t)n * 8 + (j >> 1) * 4 + (j & 1)], s);
    } else {
      const int j = k - 8;
      if (s != INT_MIN) atomicMax(&extents[(size_t)n * 8 + (j >> 1) * 4 + 2 + (j & 1)], s);
    }
  }
}

__global__ __launch_bounds__(MD_TILE) void model_diameter_kernel(const float *__restrict__ vertices, int V, int ntiles, long steps,
                                                                 unsigned *__restrict__ max_bits) {
  __shared__ float4 tile[MD_TILE];
  __shared__ unsigned red[MD_TILE / kWave];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  unsigned best = 0u;
  for (long k = blockIdx.x; k < steps; k += gridDim.x) {
    const int ti = (int)(k / ntiles), tj = (int)(k - (long)ti * ntiles);
    if (tj < ti) continue;                                               // the whole workgroup
    long i = (long)ti * MD_TILE + threadIdx.x, j = (long)tj * MD_TILE + threadIdx.x;
    i = i < V ? i : V - 1;                                               // a tail repeats the last vertex
    j = j < V ? j : V - 1;
    const float xi = vertices[i * 3 + 0], yi = vertices[i * 3 + 1], zi = vertices[i * 3 + 2];
    __syncthreads();                                                     // the previous step's readers are done with the tile
    tile[threadIdx.x] = make_float4(vertices[j * 3 + 0], vertices[j * 3 + 1], vertices[j * 3 + 2], 0.f);
    __syncthreads();
#pragma unroll 8
    for (int t = 0; t < MD_TILE; ++t) {
      const float4 q = tile[t];                                          // one address for the wave: a broadcast
      const float dx = xi - q.x, dy = yi - q.y, dz = zi - q.z;
      const float d2 = (dx * dx + dy * dy) + dz * dz;
      const unsigned b = __float_as_uint(d2);
      best = b > best ? b : best;
    }
  }
  best = best > GT_INF_BITS ? GT_INF_BITS : best;                         // a NaN pattern: not finite, counts as +inf
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned w = __shfl_xor(best, o);
    best = w > best ? w : best;
  }
  if (lane == 0) red[wave] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < MD_TILE / kWave; ++w) best = red[w] > best ? red[w] : best;
    if (best != 0u) atomicMax(max_bits, best);
  }
}

__global__ void model_diameter_root_kernel(float *__restrict__ out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) out[0] = sqrtf(out[0]);       // sqrtf(+inf) = +inf
}

}  // namespace s6d

using namespace s6d;

extern "C" int s6d_gt_visibility_f32(const float *canvas, const float *depth_test, const int32_t *test_index, const float *cams, int N,
                                     int M, int H, int W, int mx, int my, float delta, uint8_t *mask, uint8_t *mask_visib,
                                     int32_t *counts, int32_t *extents, void *stream) {
  if (N < 0 || M < 1 || H < 1 || W < 1 || mx < 0 || my < 0) return S6D_EINVAL;
  if (!(delta == delta)) return S6D_EINVAL;
  const long cplane = ((long)H + 2L * my) * ((long)W + 2L * mx);
  if (cplane > 0x7fffffffL || (long)W + 2L * mx > 0x7fffffffL) return S6D_EUNSUPPORTED;
  const long chunks = (cplane + GT_CHUNK - 1) / GT_CHUNK;
  if ((long)N * chunks > 0x7fffffffL) return S6D_EUNSUPPORTED;
  if (N == 0) return S6D_OK;
  if (!canvas || !depth_test || !test_index || !cams || !mask || !mask_visib || !counts || !extents) return S6D_EINVAL;
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(gt_fill_kernel, dim3((unsigned)((N + GT_THREADS - 1) / GT_THREADS)), dim3(GT_THREADS), 0, s, counts, extents, N);
  const int rc = launch_status();
  if (rc != S6D_OK) return rc;
  hipLaunchKernelGGL(gt_visibility_kernel, dim3((unsigned)((long)N * chunks)), dim3(GT_THREADS), 0, s, canvas, depth_test, test_index,
                     cams, M, H, W, mx, my, cplane, (int)chunks, delta, mask, mask_visib, counts, extents);
  return launch_status();
}

extern "C" int s6d_model_diameter_f32(const float *vertices, int V, float *diameter, void *stream) {
  if (V < 1) return S6D_EINVAL;
  if (!vertices || !diameter) return S6D_EINVAL;
  hipStream_t s = as_stream(stream);
  hipError_t e = hipMemsetAsync(diameter, 0, 4, s);
  if (e != hipSuccess) {
    set_hip_error(e);
    return S6D_ELAUNCH;
  }
  const int ntiles = (V + MD_TILE - 1) / MD_TILE;
  const long steps = (long)ntiles * ntiles;
  long want = MD_GRID;
  if (g_s6d_persistent_grid_limit > 0 && g_s6d_persistent_grid_limit < want) want = g_s6d_persistent_grid_limit;   // set through the ABI (tests)
  const unsigned grid = (unsigned)(steps < want ? steps : want);
  hipLaunchKernelGGL(model_diameter_kernel, dim3(grid), dim3(MD_TILE), 0, s, vertices, V, ntiles, steps,
                     reinterpret_cast<unsigned *>(diameter));
  const int rc = launch_status();
  if (rc != S6D_OK) return rc;
  hipLaunchKernelGGL(model_diameter_root_kernel, dim3(1), dim3(64), 0, s, diameter);
  return launch_status();
}
