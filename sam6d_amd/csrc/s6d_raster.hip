// Template views of a CAD mesh rendered on the device (gfx950): a compute rasteriser.  The chip has no raster pipeline and the
// reference's two renderers (BlenderProc, Render/render_custom_templates.py; pyrender over EGL, Instance_Segmentation_Model/utils/
// poses/pyrender.py) cannot run on it.  Coverage, the visible face, the model coordinate of the surface point (the reference's
// xyz_i.npy / NOCS map) and the depth are geometry and are held to an exact definition; the colour of a path-traced or OpenGL
// render cannot be reproduced, so the shading is a small DEFINED model (below), not an imitation.
//
// Inputs: vertices (V,3) f32 model units, faces (F,3) i32, colors (V,3) u8, poses (T,4,4) f32 object -> camera with OpenCV axes
// (x right, y down, z forward; translation in model units), fx fy cx cy, H x W.  All T views go through one set of launches:
//   raster_small_kernel  one lane per (view, triangle): set-up, then the lane walks the triangle's bounding box clamped to the image.
//                        A triangle whose clamped box holds more than RASTER_LARGE_BOX = 256 samples (16 x 16) is appended to a list.
//   raster_large_kernel  one workgroup of 256 lanes per listed triangle, the box's samples dealt round-robin to the lanes (without it
//                        a 12-face cube makes one lane walk a whole face).  The order of the list is whatever the appends gave;
//                        the result does not depend on it (below).
//   raster_resolve_kernel  one lane per pixel: the outputs, from the winning face alone.
//
// Fixed arithmetic (float32, every operation rounded on its own: contraction is off, `/` and sqrtf are the correctly rounded forms):
//   vertex     for pose rows (r00 r01 r02 tx; ...) and a vertex v:   X = ((r00 vx + r01 vy) + r02 vz) + tx,  Y and Z alike;
//              x = (fx X) / Z + cx,  y = (fy Y) / Z + cy;  snapped to 1/256 pixel: xi = (int)rintf(x * 256) (ties to even).
//              Pixel (u, v) is sampled at its integer coordinate (256 u, 256 v): the convention in which K projects.
//              The stage is a function of (view, vertex) alone; the kernels evaluate it where they need it, with the same bits.
//   skipping   a triangle with a vertex at Z <= znear (or a NaN), with |x * 256| or |y * 256| beyond 2^23, or with a vertex index
//              outside [0, V), is skipped whole and counted in skipped[view]; there is no clipping.  The bound keeps the integers
//              below inside int64: coordinates and samples (256 u <= 2^23: H, W <= 32768) are within +-2^23, differences within
//              2^24, an edge-function product within 2^48, an edge function and the doubled area within 2^49.
//   coverage   integers only.  orient(a, b, p) = (bx - ax)(py - ay) - (by - ay)(px - ax); A2 = orient(v0, v1, v2) is the doubled
//              area, s its sign; A2 = 0 covers nothing.  Edge k runs from a = v(k+1) to b = v(k+2) (indices mod 3), its function is
//              w_k(p) = s orient(a, b, p) and its direction (dx, dy) = s (b - a): the winding is normalised by s, there is no
//              back-face culling.  A sample is covered when every w_k > 0, or w_k = 0 on an edge with dy < 0 (a left edge) or
//              dy = 0 and dx > 0 (a top edge): of two triangles on opposite sides of a shared edge exactly one owns its samples.
//   depth      lambda_k = (float)w_k / (float)A with A = |A2| (int64 -> float32 conversions round to nearest), q_k = lambda_k / Z_k,
//              iz = (q0 + q1) + q2, Z = 1 / iz: perspective-correct.  Z > 0, so its bits order like the value.
//   visibility key = (bits(Z) << 32) | face, reduced per pixel with atomicMin on unsigned long long in a (T,H,W) workspace preset
//              to all ones: the nearest surface wins, among equal depths the lowest face index.  A minimum does not depend on the
//              order of its operands: not on scheduling, the list order or what else is in the batch.
//   resolve    from the winning face f, with q_k and iz recomputed as above:  attribute(a) = ((q0 a0 + q1 a1) + q2 a2) / iz.
//              xyz = attribute(model-space vertex) per component (never an inverted pose); depth = Z of the key;
//              albedo = attribute((float)colour) per channel; Pc = attribute(camera-space vertex (X, Y, Z));
//              n = (P1 - P0) x (P2 - P0) on the camera-space vertices (nx = e1y e2z - e1z e2y, ...), the flat face normal;
//              c = |(nx Pcx + ny Pcy) + nz Pcz| / (sqrtf((nx nx + ny ny) + nz nz) sqrtf((Pcx Pcx + Pcy Pcy) + Pcz Pcz)), min(c, 1),
//              0 where the denominator is 0: |n^ . d^| with d^ the unit vector from the surface point to the camera, where the
//              light sits (as in both reference renderers); rgb = rintf(min(max(albedo (ambient + diffuse c), 0), 255)).
//   background rgb 0, mask 0, xyz 0, depth 0, face -1; mask is 255 elsewhere.
#include "s6d_common.h"

namespace s6d {

#pragma clang fp contract(off)   // the stated float32 operations, one rounding each

constexpr int RASTER_THREADS = 256;
constexpr int RASTER_LARGE_BOX = 256;                                    // samples of the clamped box above which a workgroup shares the triangle
constexpr int RASTER_LARGE_GRID = 2048;                                  // workgroups that walk the list of large triangles
constexpr float RASTER_SNAP_LIMIT = 8388608.0f;                          // 2^23 (in 1/256 pixel)
constexpr int RASTER_MAX_SIDE = 32768;                                   // 256 * side <= 2^23
constexpr unsigned long long RASTER_EMPTY = ~0ull;

struct RasterCam {
  float fx, fy, cx, cy, znear;
};

struct RasterTri {
  long e0[3], eu[3], ev[3];                                              // w_k at pixel (u, v) = e0 + eu u + ev v
  long area;                                                             // |A2| > 0
  bool own[3];                                                           // edge k owns the samples with w_k = 0 (top-left rule)
  int idx[3];
  float cam[3][3];                                                       // camera-space vertices (X, Y, Z)
  int u0, u1, v0, v1;                                                    // clamped box, inclusive
};

__device__ __forceinline__ bool raster_vertex(const float *__restrict__ P, const float *__restrict__ v, const RasterCam &c, float *cam,
                                              int &xi, int &yi) {
  const float vx = v[0], vy = v[1], vz = v[2];
  const float X = ((P[0] * vx + P[1] * vy) + P[2] * vz) + P[3];
  const float Y = ((P[4] * vx + P[5] * vy) + P[6] * vz) + P[7];
  const float Z = ((P[8] * vx + P[9] * vy) + P[10] * vz) + P[11];
  cam[0] = X;
  cam[1] = Y;
  cam[2] = Z;
  if (!(Z > c.znear)) return false;
  const float xs = ((c.fx * X) / Z + c.cx) * 256.0f, ys = ((c.fy * Y) / Z + c.cy) * 256.0f;
  if (!(fabsf(xs) <= RASTER_SNAP_LIMIT) || !(fabsf(ys) <= RASTER_SNAP_LIMIT)) return false;
  xi = (int)rintf(xs);
  yi = (int)rintf(ys);
  return true;
}

// 1: tr is set up; 0: the triangle covers no sample of the image; -1: skipped (counted by the caller)
__device__ __forceinline__ int raster_setup(const float *__restrict__ vertices, const int *__restrict__ faces,
                                            const float *__restrict__ poses, int V, int t, int f, const RasterCam &c, int H, int W,
                                            RasterTri &tr) {
  int x[3], y[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int i = faces[(size_t)f * 3 + k];
    if (i < 0 || i >= V) return -1;
    tr.idx[k] = i;
    if (!raster_vertex(poses + (size_t)t * 16, vertices + (size_t)i * 3, c, tr.cam[k], x[k], y[k])) return -1;
  }
  const long a2 = (long)(x[1] - x[0]) * (y[2] - y[0]) - (long)(y[1] - y[0]) * (x[2] - x[0]);
  if (a2 == 0) return 0;
  const long s = a2 > 0 ? 1 : -1;
  tr.area = s * a2;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int a = (k + 1) % 3, b = (k + 2) % 3;
    const long dx = s * (x[b] - x[a]), dy = s * (y[b] - y[a]);
    tr.e0[k] = dy * x[a] - dx * y[a];
    tr.eu[k] = -dy * 256;
    tr.ev[k] = dx * 256;
    tr.own[k] = dy < 0 || (dy == 0 && dx > 0);
  }
  const int xmin = min(x[0], min(x[1], x[2])), xmax = max(x[0], max(x[1], x[2]));
  const int ymin = min(y[0], min(y[1], y[2])), ymax = max(y[0], max(y[1], y[2]));
  tr.u0 = max(0, (xmin + 255) >> 8);                                     // ceil(xmin / 256): >> floors, also below zero
  tr.u1 = min(W - 1, xmax >> 8);
  tr.v0 = max(0, (ymin + 255) >> 8);
  tr.v1 = min(H - 1, ymax >> 8);
  return (tr.u0 <= tr.u1 && tr.v0 <= tr.v1) ? 1 : 0;
}

__device__ __forceinline__ bool raster_covers(const RasterTri &tr, int u, int v, long *w) {
  bool in = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    w[k] = tr.e0[k] + tr.eu[k] * u + tr.ev[k] * v;
    in = in && (w[k] > 0 || (w[k] == 0 && tr.own[k]));
  }
  return in;
}

// q_k = lambda_k / Z_k and iz = (q0 + q1) + q2
__device__ __forceinline__ float raster_weights(const RasterTri &tr, const long *w, float *q) {
  const float fa = (float)tr.area;
#pragma unroll
  for (int k = 0; k < 3; ++k) q[k] = ((float)w[k] / fa) / tr.cam[k][2];
  return (q[0] + q[1]) + q[2];
}

// The coverage pass is one pair of kernels over two policies.  KEY: the word a covered sample leaves in the per-pixel minimum and
// how it is made from (Z, face).  CAM: where the camera of view t comes from.
struct RasterKeyFace {                                                   // the template render: visibility key of the header
  typedef unsigned long long word;
  static __device__ __forceinline__ word make(float z, int f) {
    return ((unsigned long long)__float_as_uint(z) << 32) | (unsigned long long)(unsigned)f;
  }
};
struct RasterKeyDepth {                                                  // the depth render: bits(Z) alone
  typedef unsigned word;
  static __device__ __forceinline__ word make(float z, int) { return __float_as_uint(z); }
};
struct RasterOneCam {                                                    // one camera for all views
  RasterCam c;
  __device__ __forceinline__ RasterCam view(int) const { return c; }
};
struct RasterViewCams {                                                  // cams (T,4) f32 [fx fy cx cy] and one znear
  const float *cams;
  float znear;
  __device__ __forceinline__ RasterCam view(int t) const {
    const float *k = cams + (size_t)t * 4;
    return RasterCam{k[0], k[1], k[2], k[3], znear};
  }
};

template <class KEY>
__device__ __forceinline__ void raster_sample(const RasterTri &tr, int u, int v, int f, typename KEY::word *__restrict__ key) {
  long w[3];
  if (!raster_covers(tr, u, v, w)) return;
  float q[3];
  const float z = 1.0f / raster_weights(tr, w, q);
  atomicMin(key, KEY::make(z, f));
}

template <class KEY, class CAM>
__global__ __launch_bounds__(RASTER_THREADS) void raster_small_kernel(const float *__restrict__ vertices, const int *__restrict__ faces,
                                                                      const float *__restrict__ poses, int V, int F, int T, int H, int W,
                                                                      CAM cam, typename KEY::word *__restrict__ keys,
                                                                      int *__restrict__ large_list, int *__restrict__ large_count,
                                                                      int *__restrict__ skipped) {
  const long i = (long)blockIdx.x * RASTER_THREADS + threadIdx.x;
  if (i >= (long)T * F) return;
  const int t = (int)(i / F), f = (int)(i - (long)t * F);
  const RasterCam c = cam.view(t);
  RasterTri tr;
  const int st = raster_setup(vertices, faces, poses, V, t, f, c, H, W, tr);
  if (st < 0) atomicAdd(&skipped[t], 1);
  if (st <= 0) return;
  if ((long)(tr.u1 - tr.u0 + 1) * (tr.v1 - tr.v0 + 1) > RASTER_LARGE_BOX) {
    large_list[atomicAdd(large_count, 1)] = (int)i;                      // at most T * F appends: the list's size
    return;
  }
  typename KEY::word *kp = keys + (size_t)t * H * W;
  for (int v = tr.v0; v <= tr.v1; ++v)
    for (int u = tr.u0; u <= tr.u1; ++u) raster_sample<KEY>(tr, u, v, f, kp + (size_t)v * W + u);
}

template <class KEY, class CAM>
__global__ __launch_bounds__(RASTER_THREADS) void raster_large_kernel(const float *__restrict__ vertices, const int *__restrict__ faces,
                                                                      const float *__restrict__ poses, int V, int F, int H, int W,
                                                                      CAM cam, typename KEY::word *__restrict__ keys,
                                                                      const int *__restrict__ large_list,
                                                                      const int *__restrict__ large_count) {
  const int count = *large_count;
  for (int e = blockIdx.x; e < count; e += gridDim.x) {
    const int i = large_list[e];
    const int t = i / F, f = i - t * F;
    const RasterCam c = cam.view(t);
    RasterTri tr;                                                        // every lane sets the triangle up: the same values
    if (raster_setup(vertices, faces, poses, V, t, f, c, H, W, tr) <= 0) continue;
    const int bw = tr.u1 - tr.u0 + 1;
    const long n = (long)bw * (tr.v1 - tr.v0 + 1);
    typename KEY::word *kp = keys + (size_t)t * H * W;
    for (long j = threadIdx.x; j < n; j += RASTER_THREADS) {
      const int r = (int)(j / bw), v = tr.v0 + r, u = tr.u0 + (int)(j - (long)r * bw);
      raster_sample<KEY>(tr, u, v, f, kp + (size_t)v * W + u);
    }
  }
}

__device__ __forceinline__ float raster_attribute(const float *q, float iz, float a0, float a1, float a2) {
  return ((q[0] * a0 + q[1] * a1) + q[2] * a2) / iz;
}

__global__ __launch_bounds__(RASTER_THREADS) void raster_resolve_kernel(const float *__restrict__ vertices, const int *__restrict__ faces,
                                                                        const unsigned char *__restrict__ colors,
                                                                        const float *__restrict__ poses, int V, int T, int H, int W,
                                                                        RasterCam c, float ambient, float diffuse,
                                                                        const unsigned long long *__restrict__ keys,
                                                                        unsigned char *__restrict__ rgb, unsigned char *__restrict__ mask,
                                                                        float *__restrict__ xyz, float *__restrict__ depth,
                                                                        int *__restrict__ face) {
  const size_t plane = (size_t)H * W, total = plane * T;
  for (size_t p = (size_t)blockIdx.x * RASTER_THREADS + threadIdx.x; p < total; p += (size_t)gridDim.x * RASTER_THREADS) {
    const unsigned long long key = keys[p];
    const int t = (int)(p / plane);
    const int r = (int)(p - (size_t)t * plane), v = r / W, u = r - v * W;
    const int f = (int)(unsigned)(key & 0xffffffffull);
    RasterTri tr;
    long w[3];
    // (a key is only ever written for a triangle that was set up and covers the sample: the guards keep a stray key harmless)
    if (key == RASTER_EMPTY || raster_setup(vertices, faces, poses, V, t, f, c, H, W, tr) <= 0 || !raster_covers(tr, u, v, w)) {
      rgb[p * 3 + 0] = rgb[p * 3 + 1] = rgb[p * 3 + 2] = 0;
      mask[p] = 0;
      xyz[p * 3 + 0] = xyz[p * 3 + 1] = xyz[p * 3 + 2] = 0.f;
      depth[p] = 0.f;
      face[p] = -1;
      continue;
    }
    float q[3];
    const float iz = raster_weights(tr, w, q);
    const float *m0 = vertices + (size_t)tr.idx[0] * 3, *m1 = vertices + (size_t)tr.idx[1] * 3, *m2 = vertices + (size_t)tr.idx[2] * 3;
    const unsigned char *c0 = colors + (size_t)tr.idx[0] * 3, *c1 = colors + (size_t)tr.idx[1] * 3, *c2 = colors + (size_t)tr.idx[2] * 3;
    float pc[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      xyz[p * 3 + k] = raster_attribute(q, iz, m0[k], m1[k], m2[k]);
      pc[k] = raster_attribute(q, iz, tr.cam[0][k], tr.cam[1][k], tr.cam[2][k]);
    }
    const float e1x = tr.cam[1][0] - tr.cam[0][0], e1y = tr.cam[1][1] - tr.cam[0][1], e1z = tr.cam[1][2] - tr.cam[0][2];
    const float e2x = tr.cam[2][0] - tr.cam[0][0], e2y = tr.cam[2][1] - tr.cam[0][1], e2z = tr.cam[2][2] - tr.cam[0][2];
    const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const float nd = (nx * pc[0] + ny * pc[1]) + nz * pc[2];
    const float den = sqrtf((nx * nx + ny * ny) + nz * nz) * sqrtf((pc[0] * pc[0] + pc[1] * pc[1]) + pc[2] * pc[2]);
    const float cosine = den > 0.f ? fminf(fabsf(nd) / den, 1.0f) : 0.f;
    const float shade = ambient + diffuse * cosine;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float albedo = raster_attribute(q, iz, (float)c0[k], (float)c1[k], (float)c2[k]);
      rgb[p * 3 + k] = (unsigned char)rintf(fminf(fmaxf(albedo * shade, 0.f), 255.f));
    }
    mask[p] = 255;
    depth[p] = __uint_as_float((unsigned)(key >> 32));
    face[p] = f;
  }
}

// ---- depth alone, a camera per view (s6d_raster_depth_f32: the two renders of a VSD evaluation, csrc/s6d_boperr.hip) ----------------
// raster_small_kernel / raster_large_kernel<RasterKeyDepth, RasterViewCams>: the kernels of the full render with another key and
// camera source, so a pixel holds the depth bits the full render gives it.  The key is bits(Z) alone (Z > 0: the bits order like the
// value), reduced with atomicMin on unsigned IN the depth output, preset to all ones; a last pass turns what is still all ones into 0.
// The workspace is the list of large triangles only.
constexpr unsigned RASTER_EMPTY32 = ~0u;

__global__ __launch_bounds__(RASTER_THREADS) void raster_depth_resolve_kernel(unsigned *__restrict__ keys, size_t total) {
  for (size_t p = (size_t)blockIdx.x * RASTER_THREADS + threadIdx.x; p < total; p += (size_t)gridDim.x * RASTER_THREADS)
    if (keys[p] == RASTER_EMPTY32) keys[p] = 0u;                         // the bits of 0.f: background
}

// workspace of the full render: keys (T,H,W) u64 | list (T F) i32 | the list's length (one i32, padded to 8 bytes); of the depth
// render: the list and its length
__host__ inline long raster_list_bytes(int T, int F) { return ((long)T * F * 4 + 7) & ~7L; }
__host__ inline long raster_list_offset(int T, int H, int W) { return (long)T * H * W * 8; }
__host__ inline bool raster_sizes_ok(int V, int F, int T, int H, int W) { return V >= 0 && F >= 0 && T >= 0 && H > 0 && W > 0; }
__host__ inline bool raster_sizes_supported(int F, int T, int H, int W) {
  return H <= RASTER_MAX_SIDE && W <= RASTER_MAX_SIDE && (long)T * F <= 0x7fffffffL && (long)T * H * W <= (1L << 40);
}
__host__ inline unsigned raster_resolve_grid(size_t total) {
  const size_t g = (total + RASTER_THREADS - 1) / RASTER_THREADS;
  return (unsigned)(g > 65536 ? 65536 : g);
}

// What the two renders share up to their resolve pass: keys, the list's length and `skipped` preset, then the coverage launches.
// `list` points at the list of large triangles, its length follows it.
template <class KEY, class CAM>
static int raster_cover(const float *vertices, const int32_t *faces, const float *poses, int V, int F, int T, int H, int W, CAM cam,
                        typename KEY::word *keys, char *list, int32_t *skipped, hipStream_t s) {
  int *count = reinterpret_cast<int *>(list + raster_list_bytes(T, F));
  hipError_t e = hipMemsetAsync(keys, 0xff, (size_t)T * H * W * sizeof(typename KEY::word), s);
  if (e == hipSuccess) e = hipMemsetAsync(count, 0, 8, s);
  if (e == hipSuccess) e = hipMemsetAsync(skipped, 0, (size_t)T * 4, s);
  if (e != hipSuccess) {
    set_hip_error(e);
    return S6D_ELAUNCH;
  }
  const long pairs = (long)T * F;
  if (pairs == 0) return S6D_OK;
  hipLaunchKernelGGL((raster_small_kernel<KEY, CAM>), dim3((unsigned)((pairs + RASTER_THREADS - 1) / RASTER_THREADS)),
                     dim3(RASTER_THREADS), 0, s, vertices, faces, poses, V, F, T, H, W, cam, keys, reinterpret_cast<int *>(list), count,
                     skipped);
  const int rc = launch_status();
  if (rc != S6D_OK) return rc;
  hipLaunchKernelGGL((raster_large_kernel<KEY, CAM>), dim3((unsigned)(pairs < RASTER_LARGE_GRID ? pairs : RASTER_LARGE_GRID)),
                     dim3(RASTER_THREADS), 0, s, vertices, faces, poses, V, F, H, W, cam, keys, reinterpret_cast<int *>(list), count);
  return launch_status();
}

}  // namespace s6d

using namespace s6d;

extern "C" long s6d_raster_workspace_bytes(int T, int F, int H, int W) {
  if (!raster_sizes_ok(0, F, T, H, W) || !raster_sizes_supported(F, T, H, W)) return -1;
  return raster_list_offset(T, H, W) + raster_list_bytes(T, F) + 8;
}

extern "C" int s6d_raster_views_f32(const float *vertices, const int32_t *faces, const unsigned char *colors, const float *poses, int V,
                                    int F, int T, int H, int W, float fx, float fy, float cx, float cy, float znear, float ambient,
                                    float diffuse, void *workspace, unsigned char *rgb, unsigned char *mask, float *xyz, float *depth,
                                    int32_t *face, int32_t *skipped, void *stream) {
  if (!raster_sizes_ok(V, F, T, H, W)) return S6D_EINVAL;
  const float lim = 3.402823466e+38f;
  if (!(fabsf(fx) <= lim) || !(fabsf(fy) <= lim) || !(fabsf(cx) <= lim) || !(fabsf(cy) <= lim) || !(znear >= 0.f && znear <= lim) ||
      !(fabsf(ambient) <= lim) || !(fabsf(diffuse) <= lim))
    return S6D_EINVAL;
  if (!raster_sizes_supported(F, T, H, W)) return S6D_EUNSUPPORTED;
  if (T == 0) return S6D_OK;
  if (!poses || !workspace || !rgb || !mask || !xyz || !depth || !face || !skipped || (F > 0 && (!vertices || !faces || !colors)))
    return S6D_EINVAL;
  if ((uintptr_t)workspace & 7) return S6D_EINVAL;
  hipStream_t s = as_stream(stream);
  char *ws = reinterpret_cast<char *>(workspace);
  unsigned long long *keys = reinterpret_cast<unsigned long long *>(ws);
  const RasterOneCam cam = {{fx, fy, cx, cy, znear}};
  const int rc = raster_cover<RasterKeyFace>(vertices, faces, poses, V, F, T, H, W, cam, keys, ws + raster_list_offset(T, H, W), skipped, s);
  if (rc != S6D_OK) return rc;
  hipLaunchKernelGGL(raster_resolve_kernel, dim3(raster_resolve_grid((size_t)T * H * W)), dim3(RASTER_THREADS), 0, s, vertices, faces,
                     colors, poses, V, T, H, W, cam.c, ambient, diffuse, keys, rgb, mask, xyz, depth, face);
  return launch_status();
}

extern "C" long s6d_raster_depth_workspace_bytes(int T, int F, int H, int W) {
  if (!raster_sizes_ok(0, F, T, H, W) || !raster_sizes_supported(F, T, H, W)) return -1;
  return raster_list_bytes(T, F) + 8;
}

extern "C" int s6d_raster_depth_f32(const float *vertices, const int32_t *faces, const float *poses, const float *cams, int V, int F,
                                    int T, int H, int W, float znear, void *workspace, float *depth, int32_t *skipped, void *stream) {
  if (!raster_sizes_ok(V, F, T, H, W)) return S6D_EINVAL;
  if (!(znear >= 0.f && znear <= 3.402823466e+38f)) return S6D_EINVAL;
  if (!raster_sizes_supported(F, T, H, W)) return S6D_EUNSUPPORTED;
  if (T == 0) return S6D_OK;
  if (!poses || !cams || !workspace || !depth || !skipped || (F > 0 && (!vertices || !faces))) return S6D_EINVAL;
  if ((uintptr_t)workspace & 7) return S6D_EINVAL;
  hipStream_t s = as_stream(stream);
  unsigned *keys = reinterpret_cast<unsigned *>(depth);
  const int rc = raster_cover<RasterKeyDepth>(vertices, faces, poses, V, F, T, H, W, RasterViewCams{cams, znear}, keys,
                                              reinterpret_cast<char *>(workspace), skipped, s);
  if (rc != S6D_OK) return rc;
  const size_t total = (size_t)T * H * W;
  hipLaunchKernelGGL(raster_depth_resolve_kernel, dim3(raster_resolve_grid(total)), dim3(RASTER_THREADS), 0, s, keys, total);
  return launch_status();
}
