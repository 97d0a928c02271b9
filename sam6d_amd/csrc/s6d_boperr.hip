// BOP pose errors on the device (gfx950): MSSD / MSPD of a batch of estimates of one object, and the per-pixel stage of VSD (the two
// depth renders VSD needs are s6d_raster_depth_f32, csrc/s6d_raster.hip).  bop_toolkit is not part of this project and none of its
// text is used: the errors are DEFINED here, operation by operation, in the way the rasteriser and the samplers are defined, and the
// tests pin the kernels to an independent restatement of this header (tests/bop_ref.py).  Nothing claims equality with the toolkit's
// output.
//
// Fixed arithmetic (float32, every operation rounded on its own: contraction is off, `/` and sqrtf are the correctly rounded forms).
//
// pose_err_kernel   one workgroup of 256 lanes per (estimate n, symmetry s); E = est[n], G = gts[n][s] (the ground truth already
//                   composed with the symmetry, on the host in float64, rounded once); fx fy cx cy = cams[n].
//   transform  for pose rows (r00 r01 r02 tx; ...) and a vertex v:  X = ((r00 vx + r01 vy) + r02 vz) + tx,  Y and Z alike
//              (the rasteriser's vertex statement; pose_err_transform of csrc/s6d_bopvis.h, which ADD / ADD-S share), once with E
//              and once with G.
//   MSSD       d3 = (dx dx + dy dy) + dz dz  with  dx = Xe - Xg, ...;  a d3 that is not finite (NaN included) counts as +inf.
//   MSPD       x = (fx X) / Z + cx,  y = (fy Y) / Z + cy  for both poses;  d2 = du du + dv dv  with  du = xe - xg, dv = ye - yg;
//              a vertex with Z <= 0 (or NaN) in either pose, or a d2 that is not finite, counts as +inf.
//   reduction  lanes stride over the vertices and keep the maximum of d3 and of d2 (no NaN reaches fmaxf), then the wave
//              (shuffles) and the four waves (LDS); lane 0 takes ONE sqrtf of each maximum -- sqrtf is monotone, so these are the
//              bits of the maximum of the roots -- and issues one atomicMin per output on the bits of the non-negative float, into
//              outputs a fill kernel preset to +inf's bits:  mssd[n] = min_s max_v |E v - G v|,  mspd[n] likewise in pixels.
//              Maximum and minimum do not depend on the order of their operands: an instance has the same bits alone and in a
//              batch, under any scheduling.  There is no cross-workgroup protocol other than that atomic.
//
// vsd_counts_kernel  workgroups of 256 lanes, each over a run of VSD_CHUNK pixels of ONE pair n; Ze = depth_est[n], Zg = depth_gt[n],
//                   Zt = depth_test[test_index[n]] at pixel (u, v), all camera Z in model units, 0 = nothing there.
//   ray        a = ((float)u - cx) / fx,  b = ((float)v - cy) / fy,  r = sqrtf((a a + b b) + 1);  D = Z r for the three depths:
//              the distance from the camera centre.
//   visibility vis_gt  = Zg > 0 && ((Dg - Dt) <= delta || Zt == 0)
//              vis_est = Ze > 0 && (((De - Dt) <= delta || Zt == 0) || vis_gt)          (the BOP19 rule)
//   counts     union += vis_gt || vis_est;  inter += vis_gt && vis_est;  on inter:  x = fabsf(Dg - De) / scale[n],
//              ge[n][k] += x >= taus[k]  (scale = the diameter for the normalised thresholds, 1 for plain ones).
//   reduction  integer counters per lane, summed in the wave and through LDS, one integer atomicAdd per output and workgroup into
//              zeroed outputs.  Integer sums do not depend on their order: the counts are exact and reproducible.
//              The caller forms e_k = (ge_k + union - inter) / union in float64 (1 when union = 0).
//              A test_index outside [0, M) leaves the pair's counts at zero (the wrapper refuses it on the host).
#include "s6d_bopvis.h"

namespace s6d {

#pragma clang fp contract(off)   // the stated float32 operations, one rounding each

constexpr int BE_THREADS = 256;
constexpr int BE_WAVES = BE_THREADS / kWave;
constexpr unsigned BE_INF_BITS = 0x7f800000u;
constexpr int VSD_MAX_TAUS = 16;
constexpr int VSD_CHUNK = BE_THREADS * 8;                                // pixels of one workgroup
constexpr int VSD_COUNTERS = VSD_MAX_TAUS + 2;

struct VsdTaus {
  float t[VSD_MAX_TAUS];
};

__global__ __launch_bounds__(BE_THREADS) void pose_err_fill_kernel(unsigned *__restrict__ a, unsigned *__restrict__ b, int n) {
  const int i = blockIdx.x * BE_THREADS + threadIdx.x;
  if (i < n) a[i] = b[i] = BE_INF_BITS;
}

__global__ __launch_bounds__(BE_THREADS) void pose_err_kernel(const float *__restrict__ vertices, const float *__restrict__ est,
                                                              const float *__restrict__ gts, const float *__restrict__ cams, int V,
                                                              int S, unsigned *__restrict__ mssd, unsigned *__restrict__ mspd) {
  __shared__ float red[2][BE_WAVES];
  const int pair = blockIdx.x, n = pair / S;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float E[12], G[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    E[k] = est[(size_t)n * 16 + k];
    G[k] = gts[(size_t)pair * 16 + k];
  }
  const float fx = cams[(size_t)n * 4 + 0], fy = cams[(size_t)n * 4 + 1], cx = cams[(size_t)n * 4 + 2], cy = cams[(size_t)n * 4 + 3];
  const float inf = __uint_as_float(BE_INF_BITS);
  float m3 = 0.f, m2 = 0.f;                                              // squared distances are >= 0
  for (int i = threadIdx.x; i < V; i += BE_THREADS) {
    const float vx = vertices[(size_t)i * 3 + 0], vy = vertices[(size_t)i * 3 + 1], vz = vertices[(size_t)i * 3 + 2];
    float Xe, Ye, Ze, Xg, Yg, Zg;
    pose_err_transform(E, vx, vy, vz, Xe, Ye, Ze);
    pose_err_transform(G, vx, vy, vz, Xg, Yg, Zg);
    const float dx = Xe - Xg, dy = Ye - Yg, dz = Ze - Zg;
    float d3 = (dx * dx + dy * dy) + dz * dz;
    if (!(d3 < inf)) d3 = inf;                                           // NaN too: fmaxf below would drop it
    float d2 = inf;
    if (Ze > 0.f && Zg > 0.f) {
      const float du = ((fx * Xe) / Ze + cx) - ((fx * Xg) / Zg + cx);
      const float dv = ((fy * Ye) / Ze + cy) - ((fy * Yg) / Zg + cy);
      d2 = du * du + dv * dv;
      if (!(d2 < inf)) d2 = inf;
    }
    m3 = fmaxf(m3, d3);
    m2 = fmaxf(m2, d2);
  }
  m3 = wave_max(m3);
  m2 = wave_max(m2);
  if (lane == 0) {
    red[0][wave] = m3;
    red[1][wave] = m2;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < BE_WAVES; ++w) {
      m3 = fmaxf(m3, red[0][w]);
      m2 = fmaxf(m2, red[1][w]);
    }
    atomicMin(&mssd[n], __float_as_uint(sqrtf(m3)));
    atomicMin(&mspd[n], __float_as_uint(sqrtf(m2)));
  }
}

__global__ __launch_bounds__(BE_THREADS) void vsd_counts_kernel(const float *__restrict__ depth_est, const float *__restrict__ depth_gt,
                                                                const float *__restrict__ depth_test,
                                                                const int *__restrict__ test_index, const float *__restrict__ cams,
                                                                const float *__restrict__ scale, int M, int W, long plane, int chunks,
                                                                int NT, float delta, VsdTaus taus, int *__restrict__ uni,
                                                                int *__restrict__ inter, int *__restrict__ ge) {
  __shared__ int red[VSD_COUNTERS][BE_WAVES];
  const int n = blockIdx.x / chunks, chunk = blockIdx.x - n * chunks;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ti = test_index[n];
  if (ti < 0 || ti >= M) return;                                         // the whole workgroup: nothing is read out of bounds
  const float fx = cams[(size_t)n * 4 + 0], fy = cams[(size_t)n * 4 + 1], cx = cams[(size_t)n * 4 + 2], cy = cams[(size_t)n * 4 + 3];
  const float sc = scale[n];
  const float *ZE = depth_est + (size_t)n * plane, *ZG = depth_gt + (size_t)n * plane, *ZT = depth_test + (size_t)ti * plane;
  int cnt[VSD_COUNTERS];
#pragma unroll
  for (int k = 0; k < VSD_COUNTERS; ++k) cnt[k] = 0;
  const long p0 = (long)chunk * VSD_CHUNK, p1 = p0 + VSD_CHUNK < plane ? p0 + VSD_CHUNK : plane;
  for (long p = p0 + threadIdx.x; p < p1; p += BE_THREADS) {
    const int v = (int)(p / W), u = (int)(p - (long)v * W);
    const float ze = ZE[p], zg = ZG[p], zt = ZT[p];
    const float r = bop_ray_factor(u, v, fx, fy, cx, cy);
    const float De = ze * r, Dg = zg * r, Dt = zt * r;
    const bool vis_gt = bop_visible(zg, zt, Dg, Dt, delta);          // csrc/s6d_bopvis.h: the statement gt_visibility_kernel shares
    const bool vis_est = ze > 0.f && (((De - Dt) <= delta || zt == 0.f) || vis_gt);
    cnt[0] += (vis_gt || vis_est) ? 1 : 0;
    if (vis_gt && vis_est) {
      cnt[1] += 1;
      const float x = fabsf(Dg - De) / sc;
#pragma unroll
      for (int k = 0; k < VSD_MAX_TAUS; ++k) cnt[2 + k] += (k < NT && x >= taus.t[k]) ? 1 : 0;
    }
  }
#pragma unroll
  for (int k = 0; k < VSD_COUNTERS; ++k) {
    const int s = wave_sum_i32(cnt[k]);
    if (lane == 0) red[k][wave] = s;
  }
  __syncthreads();
  if (threadIdx.x < 2 + NT) {
    const int k = threadIdx.x;
    int s = 0;
#pragma unroll
    for (int w = 0; w < BE_WAVES; ++w) s += red[k][w];
    if (s != 0) atomicAdd(k == 0 ? &uni[n] : k == 1 ? &inter[n] : &ge[(size_t)n * NT + (k - 2)], s);
  }
}

}  // namespace s6d

using namespace s6d;

extern "C" int s6d_pose_err_mssd_mspd_f32(const float *vertices, const float *est, const float *gts, const float *cams, int V, int N,
                                          int S, float *mssd, float *mspd, void *stream) {
  if (V < 1 || N < 0 || S < 1) return S6D_EINVAL;
  if ((long)N * S > 0x7fffffffL) return S6D_EUNSUPPORTED;
  if (N == 0) return S6D_OK;
  if (!vertices || !est || !gts || !cams || !mssd || !mspd) return S6D_EINVAL;
  hipStream_t s = as_stream(stream);
  unsigned *o3 = reinterpret_cast<unsigned *>(mssd), *o2 = reinterpret_cast<unsigned *>(mspd);
  hipLaunchKernelGGL(pose_err_fill_kernel, dim3((unsigned)((N + BE_THREADS - 1) / BE_THREADS)), dim3(BE_THREADS), 0, s, o3, o2, N);
  const int rc = launch_status();
  if (rc != S6D_OK) return rc;
  hipLaunchKernelGGL(pose_err_kernel, dim3((unsigned)((long)N * S)), dim3(BE_THREADS), 0, s, vertices, est, gts, cams, V, S, o3, o2);
  return launch_status();
}

extern "C" int s6d_vsd_counts_f32(const float *depth_est, const float *depth_gt, const float *depth_test, const int32_t *test_index,
                                  const float *cams, const float *scale, int N, int M, int H, int W, float delta,
                                  const float *taus_host, int NT, int32_t *uni, int32_t *inter, int32_t *ge, void *stream) {
  if (N < 0 || M < 1 || H < 1 || W < 1 || NT < 1 || NT > VSD_MAX_TAUS) return S6D_EINVAL;
  if (!(delta == delta)) return S6D_EINVAL;
  const long plane = (long)H * W;
  const long chunks = (plane + VSD_CHUNK - 1) / VSD_CHUNK;
  if (plane > 0x7fffffffL || (long)N * chunks > 0x7fffffffL) return S6D_EUNSUPPORTED;
  if (N == 0) return S6D_OK;
  if (!depth_est || !depth_gt || !depth_test || !test_index || !cams || !scale || !taus_host || !uni || !inter || !ge) return S6D_EINVAL;
  VsdTaus taus;
  for (int k = 0; k < VSD_MAX_TAUS; ++k) taus.t[k] = k < NT ? taus_host[k] : 0.f;
  hipStream_t s = as_stream(stream);
  hipError_t e = hipMemsetAsync(uni, 0, (size_t)N * 4, s);
  if (e == hipSuccess) e = hipMemsetAsync(inter, 0, (size_t)N * 4, s);
  if (e == hipSuccess) e = hipMemsetAsync(ge, 0, (size_t)N * NT * 4, s);
  if (e != hipSuccess) {
    set_hip_error(e);
    return S6D_ELAUNCH;
  }
  hipLaunchKernelGGL(vsd_counts_kernel, dim3((unsigned)((long)N * chunks)), dim3(BE_THREADS), 0, s, depth_est, depth_gt, depth_test,
                     test_index, cams, scale, M, W, plane, (int)chunks, NT, delta, taus, uni, inter, ge);
  return launch_status();
}
