// Template views of a CAD mesh rendered on the device (gfx950): a compute rasteriser.  The chip has no raster pipeline and the
// reference's two renderers (BlenderProc, Render/render_custom_templates.py; pyrender over EGL, Instance_Segmentation_Model/utils/
// poses/pyrender.py) cannot run on it.  Coverage, the visible face, the model coordinate of the surface point (the reference's
// xyz_i.npy / NOCS map) and the depth are geometry and are held to an exact definition; the colour of a path-traced or OpenGL
// render cannot be reproduced, so the shading is a small DEFINED model (below), not an imitation.
//
// Inputs: vertices (V,3) f32 model units, faces (F,3) i32, poses (T,4,4) f32 object -> camera with OpenCV axes (x right, y down,
// z forward; translation in model units), fx fy cx cy, H x W, and ONE of two albedo sources: colors (V,3) u8 per vertex, or
// uv (F,3,2) f32 per face corner with the mip pyramid of an RGB texture (s6d_raster_views_tex_f32; "texture" below).  The albedo
// is data and part of the definition; the shading stays the defined model.  All T views go through one set of launches:
//   raster_small_kernel  one lane per (view, triangle): set-up, then the lane walks the triangle's bounding box clamped to the image.
//                        A triangle whose clamped box holds more than RASTER_LARGE_BOX = 256 samples (16 x 16) is appended to a list.
//   raster_large_kernel  one workgroup of 256 lanes per listed triangle, the box's samples dealt round-robin to the lanes (without it
//                        a 12-face cube makes one lane walk a whole face).  The order of the list is whatever the appends gave;
//                        the result does not depend on it (below).
//   raster_resolve_kernel  one lane per pixel: the outputs, from the winning face alone; a template over the albedo policy
//                        (RasterAlbedoColors / RasterAlbedoTexture), as the two coverage kernels are over KEY and CAM.
//   texture_pyramid_kernel  once per object, one launch per level: level l -> level l + 1 (the first launch packs the image).
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
//
// Texture (the second albedo source; geometry is untouched: coverage, key, xyz, depth, face and skipped are the bits above):
//   pyramid    level 0 is the image, (Ht,Wt,3) u8, row 0 at the top, 1 <= Ht, Wt <= 8192.  W_(l+1) = max(1, W_l >> 1), H alike;
//              texel (i, j) of level l + 1 is, per channel, (a + b + c + d + 2) >> 2 over the columns min(2i, W_l - 1) and
//              min(2i + 1, W_l - 1) and the two rows formed the same way: integers; with an odd size the last column or row of the
//              finer level is not read.  Lmax = floor(log2(max(Wt, Ht))).  Storage: one 32-bit word per texel (r | g << 8 |
//              b << 16, the top byte 0), row-major, the levels one after another; raster_tex_level_offset gives their offsets.
//   uv         attribute(u) and attribute(v) of the corner values uv[f][k] of the winning face f (per corner: a seam needs no
//              duplicated vertices).
//   level      the three edge functions of the winning face at the samples (u + 1, v) and (u, v + 1) as well (w_k + eu_k,
//              w_k + ev_k; no coverage test there), from each q_k and iz as above and the uv there: (ux, vx), (uy, vy).
//              rho2 = +inf if a neighbour has iz <= 0 or one of the six values is not finite; otherwise
//              dxu = (ux - u0) (float)Wt, dxv = (vx - v0) (float)Ht, dyu, dyv alike (unwrapped uv, level-0 sizes),
//              rx = dxu dxu + dxv dxv, ry alike, rho2 = fmaxf(rx, ry).  e = ((bits(rho2) >> 23) & 255) - 127, the unbiased
//              exponent field; L = clamp((e + 1) >> 1, 0, Lmax) (arithmetic shift) = floor(log2(rho) + 1/2): the level switches at
//              rho2 = 2^(2L-1); zero and denormals give 0, infinity and NaN Lmax.  One level is sampled: no trilinear blend.
//   sampling   at level L of W_L x H_L texels, wrap = repeat: uw = u - floorf(u), vw = v - floorf(v); x = uw (float)W_L - 0.5f,
//              y = (1.0f - vw) (float)H_L - 0.5f (v runs upwards, as in PLY and OBJ files); x0 = floorf(x), ax = x - x0,
//              i0 = (int)x0, plus W_L if negative, i1 = i0 + 1, or 0 when that equals W_L; rows alike (y0, ay, j0, j1).
//              Per channel, t_ij the texel (column i_i, row j_j): top = t00 + ax (t10 - t00), bot = t01 + ax (t11 - t01),
//              albedo = top + ay (bot - top).  A u or v at the pixel that is not finite gives albedo 0 and reads no texel
//              (for a finite one uw is in [0, 1], so x0 is in [-1, W_L - 1]: every index lies inside the level).
//              The texture bytes are used as they are: no gamma, no alpha; vertex colours play no part.  Then rgb as above.
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

// ---- the texture: pyramid layout, its one kernel, the sample ----------------------------------------------------------------------
constexpr int RASTER_TEX_MAX_SIDE = 8192;

__host__ __device__ __forceinline__ int raster_tex_level_size(int side, int l) { return (side >> l) > 1 ? (side >> l) : 1; }
// texels in front of level l (the levels sit one after another; at most 4/3 * 8192^2 texels: 32 bits hold it)
__host__ __device__ __forceinline__ unsigned raster_tex_level_offset(int Ht, int Wt, int l) {
  unsigned o = 0;
  for (int i = 0; i < l; ++i) o += (unsigned)raster_tex_level_size(Wt, i) * (unsigned)raster_tex_level_size(Ht, i);
  return o;
}
__host__ __device__ __forceinline__ int raster_tex_lmax(int Ht, int Wt) {
  int l = 0;
  for (int m = Wt > Ht ? Wt : Ht; m > 1; m >>= 1) ++l;
  return l;
}

// l < 0: the image (Ht,Wt,3) u8 -> level 0; otherwise level l -> level l + 1.  One lane per texel written.
__global__ __launch_bounds__(RASTER_THREADS) void texture_pyramid_kernel(const unsigned char *__restrict__ image,
                                                                         unsigned *__restrict__ pyramid, int Ht, int Wt, int l) {
  if (l < 0) {
    const size_t n = (size_t)Ht * Wt;
    for (size_t p = (size_t)blockIdx.x * RASTER_THREADS + threadIdx.x; p < n; p += (size_t)gridDim.x * RASTER_THREADS)
      pyramid[p] = (unsigned)image[p * 3] | ((unsigned)image[p * 3 + 1] << 8) | ((unsigned)image[p * 3 + 2] << 16);
    return;
  }
  const int ws = raster_tex_level_size(Wt, l), hs = raster_tex_level_size(Ht, l);
  const int wd = raster_tex_level_size(Wt, l + 1), hd = raster_tex_level_size(Ht, l + 1);
  const unsigned *__restrict__ src = pyramid + raster_tex_level_offset(Ht, Wt, l);
  unsigned *__restrict__ dst = pyramid + raster_tex_level_offset(Ht, Wt, l + 1);
  const size_t n = (size_t)hd * wd;
  for (size_t p = (size_t)blockIdx.x * RASTER_THREADS + threadIdx.x; p < n; p += (size_t)gridDim.x * RASTER_THREADS) {
    const int j = (int)(p / wd), i = (int)(p - (size_t)j * wd);
    const int i0 = min(2 * i, ws - 1), i1 = min(2 * i + 1, ws - 1), j0 = min(2 * j, hs - 1), j1 = min(2 * j + 1, hs - 1);
    const unsigned a = src[(size_t)j0 * ws + i0], b = src[(size_t)j0 * ws + i1], c = src[(size_t)j1 * ws + i0], d = src[(size_t)j1 * ws + i1];
    unsigned o = 0;
#pragma unroll
    for (int k = 0; k < 24; k += 8) o |= ((((a >> k) & 255u) + ((b >> k) & 255u) + ((c >> k) & 255u) + ((d >> k) & 255u) + 2u) >> 2) << k;
    dst[p] = o;
  }
}

__device__ __forceinline__ bool raster_finite(float x) { return fabsf(x) <= 3.402823466e+38f; }   // false for NaN

// The albedo policy of the resolve kernel: where the three channel values of a covered pixel come from.
struct RasterAlbedoColors {                                              // colors (V,3) u8 per vertex
  const unsigned char *colors;
  __device__ __forceinline__ void background(size_t) const {}
  __device__ __forceinline__ void albedo(const RasterTri &tr, int, size_t, const long *, const float *q, float iz, float *a) const {
    const unsigned char *c0 = colors + (size_t)tr.idx[0] * 3, *c1 = colors + (size_t)tr.idx[1] * 3, *c2 = colors + (size_t)tr.idx[2] * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) a[k] = raster_attribute(q, iz, (float)c0[k], (float)c1[k], (float)c2[k]);
  }
};
struct RasterAlbedoTexture {                                             // uv (F,3,2) f32 per corner, the pyramid of an (Ht,Wt,3) image
  const float *uv;
  const unsigned *pyramid;
  int Ht, Wt, lmax;
  int *level;                                                            // (T,H,W) i32 or NULL: the sampled level, -1 on background
  __device__ __forceinline__ void background(size_t p) const {
    if (level) level[p] = -1;
  }
  __device__ __forceinline__ void albedo(const RasterTri &tr, int f, size_t p, const long *w, const float *q, float iz, float *a) const {
    const float *c = uv + (size_t)f * 6;
    const float a0 = c[0], b0 = c[1], a1 = c[2], b1 = c[3], a2 = c[4], b2 = c[5];
    const float u0 = raster_attribute(q, iz, a0, a1, a2), v0 = raster_attribute(q, iz, b0, b1, b2);
    float rho2;
    {
      long wn[3];
      float qn[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) wn[k] = w[k] + tr.eu[k];               // the sample (u + 1, v)
      const float izx = raster_weights(tr, wn, qn);
      const float ux = raster_attribute(qn, izx, a0, a1, a2), vx = raster_attribute(qn, izx, b0, b1, b2);
#pragma unroll
      for (int k = 0; k < 3; ++k) wn[k] = w[k] + tr.ev[k];               // the sample (u, v + 1)
      const float izy = raster_weights(tr, wn, qn);
      const float uy = raster_attribute(qn, izy, a0, a1, a2), vy = raster_attribute(qn, izy, b0, b1, b2);
      const float fw = (float)Wt, fh = (float)Ht;
      const float dxu = (ux - u0) * fw, dxv = (vx - v0) * fh, dyu = (uy - u0) * fw, dyv = (vy - v0) * fh;
      const float rx = dxu * dxu + dxv * dxv, ry = dyu * dyu + dyv * dyv;
      const bool ok = !(izx <= 0.f) && !(izy <= 0.f) && raster_finite(u0) && raster_finite(v0) && raster_finite(ux) &&
                      raster_finite(vx) && raster_finite(uy) && raster_finite(vy);
      rho2 = ok ? fmaxf(rx, ry) : __uint_as_float(0x7f800000u);
    }
    const int e = (int)((__float_as_uint(rho2) >> 23) & 255u) - 127;
    const int L = min(max((e + 1) >> 1, 0), lmax);
    if (level) level[p] = L;
    if (!raster_finite(u0) || !raster_finite(v0)) {
      a[0] = a[1] = a[2] = 0.f;
      return;
    }
    const int wl = raster_tex_level_size(Wt, L), hl = raster_tex_level_size(Ht, L);
    const float uw = u0 - floorf(u0), vw = v0 - floorf(v0);
    const float x = uw * (float)wl - 0.5f, y = (1.0f - vw) * (float)hl - 0.5f;
    const float x0 = floorf(x), y0 = floorf(y), ax = x - x0, ay = y - y0;
    int i0 = (int)x0, j0 = (int)y0;
    if (i0 < 0) i0 += wl;
    if (j0 < 0) j0 += hl;
    const int i1 = i0 + 1 == wl ? 0 : i0 + 1, j1 = j0 + 1 == hl ? 0 : j0 + 1;
    const unsigned *__restrict__ t = pyramid + raster_tex_level_offset(Ht, Wt, L);
    const unsigned t00 = t[(size_t)j0 * wl + i0], t10 = t[(size_t)j0 * wl + i1], t01 = t[(size_t)j1 * wl + i0], t11 = t[(size_t)j1 * wl + i1];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float f00 = (float)((t00 >> (8 * k)) & 255u), f10 = (float)((t10 >> (8 * k)) & 255u);
      const float f01 = (float)((t01 >> (8 * k)) & 255u), f11 = (float)((t11 >> (8 * k)) & 255u);
      const float top = f00 + ax * (f10 - f00), bot = f01 + ax * (f11 - f01);
      a[k] = top + ay * (bot - top);
    }
  }
};

template <class ALBEDO>
__global__ __launch_bounds__(RASTER_THREADS) void raster_resolve_kernel(const float *__restrict__ vertices, const int *__restrict__ faces,
                                                                        ALBEDO alb, const float *__restrict__ poses, int V, int T, int H,
                                                                        int W, RasterCam c, float ambient, float diffuse,
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
      alb.background(p);
      continue;
    }
    float q[3];
    const float iz = raster_weights(tr, w, q);
    const float *m0 = vertices + (size_t)tr.idx[0] * 3, *m1 = vertices + (size_t)tr.idx[1] * 3, *m2 = vertices + (size_t)tr.idx[2] * 3;
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
    float albedo[3];
    alb.albedo(tr, f, p, w, q, iz, albedo);
#pragma unroll
    for (int k = 0; k < 3; ++k) rgb[p * 3 + k] = (unsigned char)rintf(fminf(fmaxf(albedo[k] * shade, 0.f), 255.f));
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

// What the two full renders share: the argument checks (`albedo_ok`: the operands of the albedo source), coverage, resolve.
template <class ALBEDO>
static int raster_views(const float *vertices, const int32_t *faces, ALBEDO alb, bool albedo_ok, const float *poses, int V, int F, int T,
                        int H, int W, float fx, float fy, float cx, float cy, float znear, float ambient, float diffuse, void *workspace,
                        unsigned char *rgb, unsigned char *mask, float *xyz, float *depth, int32_t *face, int32_t *skipped, void *stream) {
  if (!raster_sizes_ok(V, F, T, H, W)) return S6D_EINVAL;
  const float lim = 3.402823466e+38f;
  if (!(fabsf(fx) <= lim) || !(fabsf(fy) <= lim) || !(fabsf(cx) <= lim) || !(fabsf(cy) <= lim) || !(znear >= 0.f && znear <= lim) ||
      !(fabsf(ambient) <= lim) || !(fabsf(diffuse) <= lim))
    return S6D_EINVAL;
  if (!raster_sizes_supported(F, T, H, W)) return S6D_EUNSUPPORTED;
  if (T == 0) return S6D_OK;
  if (!poses || !workspace || !rgb || !mask || !xyz || !depth || !face || !skipped || (F > 0 && (!vertices || !faces || !albedo_ok)))
    return S6D_EINVAL;
  if ((uintptr_t)workspace & 7) return S6D_EINVAL;
  hipStream_t s = as_stream(stream);
  char *ws = reinterpret_cast<char *>(workspace);
  unsigned long long *keys = reinterpret_cast<unsigned long long *>(ws);
  const RasterOneCam cam = {{fx, fy, cx, cy, znear}};
  const int rc = raster_cover<RasterKeyFace>(vertices, faces, poses, V, F, T, H, W, cam, keys, ws + raster_list_offset(T, H, W), skipped, s);
  if (rc != S6D_OK) return rc;
  hipLaunchKernelGGL(raster_resolve_kernel<ALBEDO>, dim3(raster_resolve_grid((size_t)T * H * W)), dim3(RASTER_THREADS), 0, s, vertices,
                     faces, alb, poses, V, T, H, W, cam.c, ambient, diffuse, keys, rgb, mask, xyz, depth, face);
  return launch_status();
}

static bool raster_tex_sizes_ok(int Ht, int Wt) { return Ht >= 1 && Wt >= 1 && Ht <= RASTER_TEX_MAX_SIDE && Wt <= RASTER_TEX_MAX_SIDE; }

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
  return raster_views(vertices, faces, RasterAlbedoColors{colors}, colors != nullptr, poses, V, F, T, H, W, fx, fy, cx, cy, znear, ambient,
                      diffuse, workspace, rgb, mask, xyz, depth, face, skipped, stream);
}

extern "C" long s6d_texture_pyramid_bytes(int Ht, int Wt) {
  if (!raster_tex_sizes_ok(Ht, Wt)) return -1;
  return 4L * raster_tex_level_offset(Ht, Wt, raster_tex_lmax(Ht, Wt) + 1);
}

extern "C" int s6d_texture_pyramid_u8(const unsigned char *image, int Ht, int Wt, void *pyramid, void *stream) {
  if (!raster_tex_sizes_ok(Ht, Wt) || !image || !pyramid || ((uintptr_t)pyramid & 3)) return S6D_EINVAL;
  hipStream_t s = as_stream(stream);
  const int lmax = raster_tex_lmax(Ht, Wt);
  for (int l = -1; l < lmax; ++l) {                                      // in stream order: each launch reads what the one before wrote
    const size_t n = (size_t)raster_tex_level_size(Wt, l + 1) * raster_tex_level_size(Ht, l + 1);
    hipLaunchKernelGGL(texture_pyramid_kernel, dim3(raster_resolve_grid(n)), dim3(RASTER_THREADS), 0, s, image,
                       reinterpret_cast<unsigned *>(pyramid), Ht, Wt, l);
    const int rc = launch_status();
    if (rc != S6D_OK) return rc;
  }
  return S6D_OK;
}

extern "C" int s6d_raster_views_tex_f32(const float *vertices, const int32_t *faces, const float *uv, const void *pyramid,
                                        const float *poses, int V, int F, int T, int H, int W, int Ht, int Wt, float fx, float fy, float cx,
                                        float cy, float znear, float ambient, float diffuse, void *workspace, unsigned char *rgb,
                                        unsigned char *mask, float *xyz, float *depth, int32_t *face, int32_t *level, int32_t *skipped,
                                        void *stream) {
  if (!raster_tex_sizes_ok(Ht, Wt) || ((uintptr_t)pyramid & 3)) return S6D_EINVAL;
  const RasterAlbedoTexture alb = {uv, reinterpret_cast<const unsigned *>(pyramid), Ht, Wt, raster_tex_lmax(Ht, Wt), level};
  return raster_views(vertices, faces, alb, uv != nullptr && pyramid != nullptr, poses, V, F, T, H, W, fx, fy, cx, cy, znear, ambient,
                      diffuse, workspace, rgb, mask, xyz, depth, face, skipped, stream);
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
