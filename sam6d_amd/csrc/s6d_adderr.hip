// ADD and ADD-S pose errors on the device (gfx950): for a batch of (estimate, ground truth) pose pairs of ONE object, the distance of
// every model vertex under the two poses (ADD), its distance to the NEAREST vertex under the other pose (ADD-S), and per pair the
// mean and the maximum of each.  These definitions are this project's own: they are stated here operation by operation, the tests
// pin the kernels to an independent restatement of this header (tests/add_ref.py), and no equality with bop_toolkit or any other
// tool is claimed.
//
// Fixed arithmetic (float32, every operation rounded on its own: contraction is off, sqrtf is the correctly rounded form).
// E = est[n], G = gts[n]: 4 x 4 poses, object -> camera, model units; v_i the V vertices.
//
//   transform   X = ((r00 vx + r01 vy) + r02 vz) + tx,  Y and Z alike: pose_err_transform of csrc/s6d_bopvis.h, the one statement
//               MSSD / MSPD use too.
//   ADD         a_i = sqrtf((dx dx + dy dy) + dz dz)  with  d = E v_i - G v_i.
//   ADD-S       m_i = min_j d2(E v_i, G v_j),  d2 = (dx dx + dy dy) + dz dz;  s_i = sqrtf(m_i).  The minimum is taken on the BITS as
//               unsigned integers (d2 is never negative, so that is the float order), and every d2 that is not finite, NaN patterns
//               included, counts as +inf's bits.  The clamp is monotone on the bits, so clamping the minimum once is clamping every
//               operand: the loop carries no clamp.  No argmin is returned (ties would make it depend on the order).
//               An a_i whose squared distance is not finite is +inf as well, so s_i <= a_i holds on the bits: pair (i, i) is a
//               candidate computed by the same statement.
//   per pair    add[n] = (sum_i (double)a_i) / (double)V,  adds[n] likewise over s_i, in float64 with a FIXED order (the one
//               csrc/s6d_refine.hip states): lane l of a 256-lane workgroup adds i = l, l + 256, ... in visiting order from +0; the
//               wave by the xor butterfly x += shuffle_xor(x, o), o = 32, 16, 8, 4, 2, 1; the waves in order ((w0 + w1) + w2) + w3.
//               One workgroup per pair, no floating-point atomics.  max[n] = max_i on the bits (for ADD-S the one-sided Hausdorff
//               distance).  A per-vertex value that is not finite is +inf, never NaN, so the mean is +inf then.
//
// Bits independent of tiling: the per-vertex values are ALWAYS materialised, in (N, V) float32 -- the caller's output or the
// workspace -- and row_mean_max_kernel reads them.  The shape of the all-pairs kernel (tile, source vertices per lane, grid) can
// therefore be tuned without changing a bit of any result, and an estimate has the same bits alone, in a batch and under any
// chunking over N.
//
// add_dist_kernel       one lane per (n, i).
// adds_nearest_kernel   the hot path: V^2 pairs per estimate.  One workgroup = one estimate and a block of 256 SPL source vertices;
//                   each lane keeps its SPL source vertices, transformed by E, in registers.  The target vertices are walked in
//                   tiles of 256, each transformed by G while it is stored to LDS as (x, y, z, -); every lane reads the same LDS
//                   address (a broadcast, no bank conflict), one 16-byte read per 9 SPL lane operations.  A tail tile repeats the
//                   last target vertex, which adds only pairs that exist; tail SOURCE lanes compute on the last vertex and write
//                   nothing.  Each source vertex is owned by one lane: no atomics at all.  SPL (1, 2, 4) is a template parameter;
//                   s6d_set_adds_sources_per_lane picks it (0 = the measured default, profiles/add_eval.md).
// row_mean_max_kernel   the fixed-order float64 mean and the bit-maximum of a row of per-vertex values.
#include "s6d_bopvis.h"

namespace s6d {

#pragma clang fp contract(off)   // the stated float32 operations, one rounding each

constexpr int AD_THREADS = 256;
constexpr int AD_WAVES = AD_THREADS / kWave;
constexpr int AD_TILE = 256;constexpr unsigned AD_INF_BITS = 0x7f800000u;
constexpr long AD_MIN_GRID = 1024;                                       // workgroups the default sources-per-lane choice keeps: 4 per CU

int g_s6d_adds_spl = 0;

__global__ __launch_bounds__(AD_THREADS) void add_dist_kernel(const float *__restrict__ vertices, const float *__restrict__ est,
                                                              const float *__restrict__ gts, int V, int vblocks,
                                                              float *__restrict__ per_vertex) {
  const int n = blockIdx.x / vblocks, vb = blockIdx.x - n * vblocks;
  const int i = vb * AD_THREADS + threadIdx.x;
  if (i >= V) return;
  float E[12], G[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    E[k] = est[(size_t)n * 16 + k];
    G[k] = gts[(size_t)n * 16 + k];
  }
  const float vx = vertices[(size_t)i * 3 + 0], vy = vertices[(size_t)i * 3 + 1], vz = vertices[(size_t)i * 3 + 2];
  float Xe, Ye, Ze, Xg, Yg, Zg;
  pose_err_transform(E, vx, vy, vz, Xe, Ye, Ze);
  pose_err_transform(G, vx, vy, vz, Xg, Yg, Zg);
  const float dx = Xe - Xg, dy = Ye - Yg, dz = Ze - Zg;
  unsigned b = __float_as_uint((dx * dx + dy * dy) + dz * dz);
  b = b > AD_INF_BITS ? AD_INF_BITS : b;                                 // not finite, NaN patterns included: +inf
  per_vertex[(size_t)n * V + i] = sqrtf(__uint_as_float(b));
}

template <int SPL>
__global__ __launch_bounds__(AD_THREADS) void adds_nearest_kernel(const float *__restrict__ vertices, const float *__restrict__ est,
                                                                  const float *__restrict__ gts, int V, int sblocks,
                                                                  float *__restrict__ per_vertex) {
  __shared__ float4 tile[AD_TILE];
  const int n = blockIdx.x / sblocks, sb = blockIdx.x - n * sblocks;
  float E[12], G[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    E[k] = est[(size_t)n * 16 + k];
    G[k] = gts[(size_t)n * 16 + k];
  }
  const long base = (long)sb * (AD_TILE * SPL) + threadIdx.x;            // this lane's sources: base, base + 256, ...
  float sx[SPL], sy[SPL], sz[SPL];
  unsigned best[SPL];
#pragma unroll
  for (int k = 0; k < SPL; ++k) {
    long i = base + (long)k * AD_TILE;
    i = i < V ? i : V - 1;                                               // a tail lane: the last vertex, nothing written below
    pose_err_transform(E, vertices[i * 3 + 0], vertices[i * 3 + 1], vertices[i * 3 + 2], sx[k], sy[k], sz[k]);
    best[k] = 0xffffffffu;
  }
  const int ntiles = (V + AD_TILE - 1) / AD_TILE;
  long j = threadIdx.x < V ? threadIdx.x : V - 1;
  float nx = vertices[j * 3 + 0], ny = vertices[j * 3 + 1], nz = vertices[j * 3 + 2];
  for (int tj = 0; tj < ntiles; ++tj) {
    float X, Y, Z;
    pose_err_transform(G, nx, ny, nz, X, Y, Z);
    __syncthreads();                                                     // the previous tile's readers are done
    tile[threadIdx.x] = make_float4(X, Y, Z, 0.f);
    __syncthreads();
    if (tj + 1 < ntiles) {                                               // the next tile's vertex travels while this one is read
      j = (long)(tj + 1) * AD_TILE + threadIdx.x;
      j = j < V ? j : V - 1;                                             // a tail repeats the last vertex
      nx = vertices[j * 3 + 0], ny = vertices[j * 3 + 1], nz = vertices[j * 3 + 2];
    }
#pragma unroll 8
    for (int t = 0; t < AD_TILE; ++t) {                                  // the loop shape of model_diameter_kernel (csrc/s6d_bopgt.hip)
      const float4 q = tile[t];                                          // one address for the wave: a broadcast
#pragma unroll
      for (int k = 0; k < SPL; ++k) {
        const float dx = sx[k] - q.x, dy = sy[k] - q.y, dz = sz[k] - q.z;
        const unsigned b = __float_as_uint((dx * dx + dy * dy) + dz * dz);
        best[k] = b < best[k] ? b : best[k];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < SPL; ++k) {
    const long i = base + (long)k * AD_TILE;
    if (i < V) {
      const unsigned b = best[k] > AD_INF_BITS ? AD_INF_BITS : best[k];  // the clamp of every operand, taken once (monotone)
      per_vertex[(size_t)n * V + i] = sqrtf(__uint_as_float(b));
    }
  }
}

__device__ __forceinline__ double ad_wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ __launch_bounds__(AD_THREADS) void row_mean_max_kernel(const float *__restrict__ values, int V, double *__restrict__ mean,
                                                                  float *__restrict__ vmax) {
  __shared__ double red[AD_WAVES];
  __shared__ unsigned redm[AD_WAVES];
  const int n = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float *row = values + (size_t)n * V;
  double acc = 0.0;
  unsigned top = 0u;
  for (int i = threadIdx.x; i < V; i += AD_THREADS) {
    const float x = row[i];
    acc = acc + (double)x;
    const unsigned b = __float_as_uint(x);
    top = b > top ? b : top;
  }
  acc = ad_wave_sum_f64(acc);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned w = __shfl_xor(top, o);
    top = w > top ? w : top;
  }
  if (lane == 0) {
    red[wave] = acc;
    redm[wave] = top;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = red[0];
#pragma unroll
    for (int w = 1; w < AD_WAVES; ++w) {
      s = s + red[w];
      top = redm[w] > top ? redm[w] : top;
    }
    mean[n] = s / (double)V;
    vmax[n] = __uint_as_float(top);
  }
}

// the checks the two entry points share; *values = where the per-vertex values go
static int ad_check(const float *vertices, int V, const float *est, const float *gts, int N, float *per_vertex, double *mean,
                    float *vmax, void *workspace, float **values) {
  if (V < 1 || N < 0) return S6D_EINVAL;
  if ((long)N * V > 0x7fffffffL) return S6D_EUNSUPPORTED;
  if (N == 0) return S6D_OK;
  if (!vertices || !est || !gts || !mean || !vmax || (!per_vertex && !workspace)) return S6D_EINVAL;
  *values = per_vertex ? per_vertex : static_cast<float *>(workspace);
  return S6D_OK;
}

static int ad_mean_max(const float *values, int V, int N, double *mean, float *vmax, hipStream_t s) {
  hipLaunchKernelGGL(row_mean_max_kernel, dim3((unsigned)N), dim3(AD_THREADS), 0, s, values, V, mean, vmax);
  return launch_status();
}

}  // namespace s6d

using namespace s6d;

extern "C" int s6d_set_adds_sources_per_lane(int sources) {
  if (sources != 0 && sources != 1 && sources != 2 && sources != 4) return S6D_EINVAL;
  g_s6d_adds_spl = sources;
  return S6D_OK;
}

extern "C" long s6d_pose_err_adds_workspace_bytes(int N, int V) {
  if (V < 1 || N < 0 || (long)N * V > 0x7fffffffL) return -1;
  return (long)N * V * 4;
}

extern "C" int s6d_pose_err_add_f32(const float *vertices, int V, const float *est, const float *gts, int N, float *per_vertex,
                                    double *mean, float *max, void *workspace, void *stream) {
  float *values = nullptr;
  const int rc = ad_check(vertices, V, est, gts, N, per_vertex, mean, max, workspace, &values);
  if (rc != S6D_OK || N == 0) return rc;
  const long vblocks = ((long)V + AD_THREADS - 1) / AD_THREADS;
  if ((long)N * vblocks > 0x7fffffffL) return S6D_EUNSUPPORTED;
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(add_dist_kernel, dim3((unsigned)((long)N * vblocks)), dim3(AD_THREADS), 0, s, vertices, est, gts, V, (int)vblocks,
                     values);
  const int rl = launch_status();
  if (rl != S6D_OK) return rl;
  return ad_mean_max(values, V, N, mean, max, s);
}

extern "C" int s6d_pose_err_adds_f32(const float *vertices, int V, const float *est, const float *gts, int N, float *per_vertex,
                                     double *mean, float *max, void *workspace, void *stream) {
  float *values = nullptr;
  const int rc = ad_check(vertices, V, est, gts, N, per_vertex, mean, max, workspace, &values);
  if (rc != S6D_OK || N == 0) return rc;
  // the library's choice (profiles/add_eval.md): four sources per lane are the fastest wherever they still leave AD_MIN_GRID
  // workgroups, four per CU; below that more, smaller workgroups win
  int spl = g_s6d_adds_spl;
  if (spl == 0)
    for (spl = 4; spl > 1 && (long)N * (((long)V + AD_TILE * spl - 1) / (AD_TILE * spl)) < AD_MIN_GRID; spl >>= 1) {
    }
  const long per_block = (long)AD_TILE * spl;
  const long sblocks = ((long)V + per_block - 1) / per_block;
  if ((long)N * sblocks > 0x7fffffffL) return S6D_EUNSUPPORTED;
  hipStream_t s = as_stream(stream);
  const dim3 grid((unsigned)((long)N * sblocks)), block(AD_THREADS);
  if (spl == 1)
    hipLaunchKernelGGL(adds_nearest_kernel<1>, grid, block, 0, s, vertices, est, gts, V, (int)sblocks, values);
  else if (spl == 2)
    hipLaunchKernelGGL(adds_nearest_kernel<2>, grid, block, 0, s, vertices, est, gts, V, (int)sblocks, values);
  else
    hipLaunchKernelGGL(adds_nearest_kernel<4>, grid, block, 0, s, vertices, est, gts, V, (int)sblocks, values);
  const int rl = launch_status();
  if (rl != S6D_OK) return rl;
  return ad_mean_max(values, V, N, mean, max, s);
}
