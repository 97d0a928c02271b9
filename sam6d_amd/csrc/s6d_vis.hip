// Overlay pictures on the device (gfx950): detections and poses drawn over the frame.  The reference ends its
// demo with two pictures drawn on the host with cv2, skimage, scipy and distinctipy, one cv2 call per line or circle; none of these
// is part of this project and none of their text is used.  The pictures are DEFINED here, operation by operation, in integers; the
// tests pin the kernels to an independent restatement of this header (tests/vis_ref.py).  No picture is claimed to equal cv2's.
//
// Base image       image (B,H,W,3) uint8.  gray: every channel becomes (4899 R + 9617 G + 1868 B + 8192) >> 14; otherwise as it is.
//
// Owner map        owner (B,H,W) int32, -1 = none.
//   from masks     vis_owner_kernel, a lane per pixel.  The detections of all frames are ONE list of N masks in the words of
//                  s6d_mask_pack_u8 (bit k of word j = row-major pixel 64 j + k).  order (K) int32, K <= N, holds the detection indices frame
//                  by frame, inside a frame in rank order (score descending, then index ascending: made by the caller);
//                  frame_start (B + 1) int64 delimits the frames in it.  owner = the first detection of the frame's run whose bit
//                  is set, as its index in the list of N; an entry of order outside [0, N) is passed over.  The 64 lanes of a row
//                  segment read the same one or two words: a broadcast.
//   from layers    vis_merge_kernel, a lane per pixel and a loop over the chunk's T layers: depth (T,H,W) f32 and rgb (T,H,W,3)
//                  uint8 of s6d_raster_views_f32, frame (T) int32, instance index = first + t.  Canvas (B,H,W): zbuf f32, owner
//                  int32, shade uint8 x 3; the empty canvas is owner = -1, zbuf = 0, shade = 0.  A layer pixel with !(z > 0) is
//                  background.  The candidate (z, index) replaces the canvas's (zbuf, owner) when the canvas has no owner, z is
//                  smaller, or z is equal and the index lower: the minimum of a total order, so the canvas has the same bits for
//                  any chunking and any order of the layers.  A layer whose frame is not the pixel's is passed over.
//
// Paint            vis_paint_kernel, a workgroup of 256 lanes per tile of VIS_TH x VIS_TW pixels, a lane per four pixels of a row.
//   blend          alpha in 1/256 units, 0 .. 256.  A pixel with an owner, per channel: out = (alpha c + (256 - alpha) base + 128)
//                  >> 8, c = colors[min(owner, n_ids - 1)] or, in surface mode (shade given), shade at the pixel.  Without an
//                  owner: out = base.
//   contour        a pixel is a contour pixel when it has an owner and some 4-neighbour INSIDE the image has another owner (-1
//                  counts as another owner; neighbours outside the image do not count).
//   edge           edge_width = w, 0 <= w <= 4: pixel (x, y) takes the edge colour when any (x - i, y - j), 0 <= i, j < w, inside
//                  the image is a contour pixel; w = 0 draws none.  The owner ids of the tile and a halo (VIS_HALO = 4 to the left
//                  and above, 1 to the right and below; -2 = outside the image) sit in LDS, the contour flags of the tile and of
//                  the w - 1 pixels to its left and above after them, and the w x w dilation reads those.
//   stores         where W % 4 == 0 (and the operands are 4-byte aligned) a lane's four pixels are twelve aligned bytes: three dword
//                  loads and stores; otherwise bytes.
//
// Projection       vis_project_kernel, a lane per point: points (M,3) f32, inst (M) int32 into N instances, R (N,9) f32 row-major,
//                  t (N,3), cams (N,4) = fx fy cx cy.  float32, contraction off, every operation rounded on its own:
//                  xc = ((r00 x + r01 y) + r02 z) + tx, likewise yc, zc;  u = (fx xc) / zc + cx,  v = (fy yc) / zc + cy;
//                  valid = zc >= znear and u, v finite;  pixel = floorf, then clamped to [-8192, 8191].  An invalid point has
//                  pixel (0, 0) and flag 0; so has a point whose inst lies outside [0, N).
//
// Primitives       prims (P,8) int32 = frame, x0, y0, x1, y1, size (0 .. 64), colour (r | g << 8 | b << 16), valid: ONE list for
//                  the batch, sorted by frame (frame_start (B + 1) int64; the caller's stable sort keeps the list order inside a
//                  frame).  a = (x0, y0), b = (x1, y1), d = b - a, L = d.d, uu = (p - a).d, all int64:
//                  L = 0 or uu <= 0: covered iff 4 |p - a|^2 <= size^2;  uu >= L: iff 4 |p - b|^2 <= size^2;  otherwise iff
//                  4 cross(p - a, d)^2 <= size^2 L.  Coordinates lie in [-8192, 8191] and H, W <= 8192 (larger: S6D_EUNSUPPORTED),
//                  so every term stays below 2^61.  A disc of radius r is a = b, size = 2 r.  An entry with valid = 0, a size
//                  outside [0, 64], a coordinate outside the clamp or another frame's number covers nothing.  Painter's order: a
//                  pixel takes the colour of the covering primitive with the HIGHEST list index, opaque.
//   vis_draw_kernel  a workgroup of 256 lanes per tile of VIS_DH x VIS_DW pixels, a lane per pixel.  The frame's primitives go by in
//                  chunks of S6D_VIS_DRAW_CHUNK (a lane per primitive): "bounding box inflated by ceil(size / 2) meets the tile",
//                  the hits compacted IN LIST ORDER into LDS (wave ballot ranks + the prefix over the four waves, as block_rank of
//                  s6d_compact.h), then every pixel runs the exact test over the compacted hits and keeps the last one.  Chunks go
//                  forwards, so the last hit of the last chunk wins.  Drawn in place.
#include "s6d_common.h"

namespace s6d {

#pragma clang fp contract(off)   // the stated float32 operations, one rounding each

constexpr int VIS_THREADS = 256;
constexpr int VIS_TH = 16, VIS_TW = 64;                                  // paint tile: a lane per 4 pixels of a row
constexpr int VIS_HALO = 4;                                              // owner ids kept left of / above the tile (edge_width <= 4)
constexpr int VIS_OH = VIS_TH + VIS_HALO + 1, VIS_OW = VIS_TW + VIS_HALO + 1;
constexpr int VIS_CH = VIS_TH + VIS_HALO - 1, VIS_CW = VIS_TW + VIS_HALO - 1;      // contour flags: the tile and 3 to the left / above
constexpr int VIS_DH = 8, VIS_DW = 32;                                   // draw tile: a lane per pixel
constexpr int VIS_CLAMP_LO = -8192, VIS_CLAMP_HI = 8191;
constexpr int VIS_MAX_HW = 8192;
static_assert(VIS_TH * VIS_TW == 4 * VIS_THREADS && VIS_DH * VIS_DW == VIS_THREADS && S6D_VIS_DRAW_CHUNK == VIS_THREADS, "tiles");

__global__ __launch_bounds__(VIS_THREADS) void vis_owner_kernel(const unsigned long long *__restrict__ packed,
                                                                const int *__restrict__ order, const long *__restrict__ frame_start,
                                                                int N, long K, long plane, long words, int blocks, int *__restrict__ owner) {
  const int b = blockIdx.x / blocks;
  const long p = (long)(blockIdx.x - b * blocks) * VIS_THREADS + threadIdx.x;
  if (p >= plane) return;
  const long j = p >> 6;
  const int bit = (int)(p & 63);
  long k0 = frame_start[b], k1 = frame_start[b + 1];                  // clamped to the list: nothing is read outside order (K)
  k0 = k0 < 0 ? 0 : k0;
  k1 = k1 > K ? K : k1;
  int own = -1;
  for (long k = k0; k < k1; ++k) {
    const int n = order[k];
    if (n < 0 || n >= N) continue;
    if ((packed[(size_t)n * words + j] >> bit) & 1ull) {
      own = n;
      break;
    }
  }
  owner[(size_t)b * plane + p] = own;
}

__global__ __launch_bounds__(VIS_THREADS) void vis_merge_kernel(const float *__restrict__ depth, const uint8_t *__restrict__ rgb,
                                                                const int *__restrict__ frame, int T, int first, long plane, int blocks,
                                                                float *__restrict__ zbuf, int *__restrict__ owner,
                                                                uint8_t *__restrict__ shade) {
  const int b = blockIdx.x / blocks;
  const long p = (long)(blockIdx.x - b * blocks) * VIS_THREADS + threadIdx.x;
  if (p >= plane) return;
  const size_t q = (size_t)b * plane + p;
  float zb = zbuf[q];
  int own = owner[q];
  int from = -1;
  for (int t = 0; t < T; ++t) {
    if (frame[t] != b) continue;                                         // the whole workgroup
    const float z = depth[(size_t)t * plane + p];
    if (!(z > 0.f)) continue;
    const int idx = first + t;
    if (own < 0 || z < zb || (z == zb && idx < own)) {
      zb = z;
      own = idx;
      from = t;
    }
  }
  if (from >= 0) {
    zbuf[q] = zb;
    owner[q] = own;
    const uint8_t *c = rgb + ((size_t)from * plane + p) * 3;
    shade[q * 3 + 0] = c[0];
    shade[q * 3 + 1] = c[1];
    shade[q * 3 + 2] = c[2];
  }
}

__device__ __forceinline__ unsigned vis_gray(unsigned r, unsigned g, unsigned b) { return (4899u * r + 9617u * g + 1868u * b + 8192u) >> 14; }

__device__ __forceinline__ unsigned vis_blend(unsigned c, unsigned base, unsigned alpha) { return (alpha * c + (256u - alpha) * base + 128u) >> 8; }

__global__ __launch_bounds__(VIS_THREADS) void vis_paint_kernel(const uint8_t *__restrict__ image, const int *__restrict__ owner,
                                                                const uint8_t *__restrict__ colors, const uint8_t *__restrict__ shade,
                                                                int n_ids, int H, int W, int tiles_x, int tiles_y, int gray, int alpha, int w,
                                                                unsigned edge_rgb, int wide, uint8_t *__restrict__ out) {
  __shared__ int own[VIS_OH][VIS_OW];
  __shared__ uint8_t cont[VIS_CH][VIS_CW + 1];
  const int tiles = tiles_x * tiles_y;
  const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int y0 = ty * VIS_TH, x0 = tx * VIS_TW;
  const size_t plane = (size_t)H * W;
  const int *OW = owner + (size_t)b * plane;
  // owner ids of the tile and its halo; -2 = outside the image
  for (int i = threadIdx.x; i < VIS_OH * VIS_OW; i += VIS_THREADS) {
    const int r = i / VIS_OW, c = i - r * VIS_OW;
    const int y = y0 - VIS_HALO + r, x = x0 - VIS_HALO + c;
    int v = -2;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      v = OW[(size_t)y * W + x];
      v = v < 0 ? -1 : v;
    }
    own[r][c] = v;
  }
  __syncthreads();
  // contour flags of the tile and of the 3 pixels to its left and above: flag (r, c) is pixel (y0 - 3 + r, x0 - 3 + c) = own[r + 1][c + 1]
  for (int i = threadIdx.x; i < VIS_CH * VIS_CW; i += VIS_THREADS) {
    const int r = i / VIS_CW, c = i - r * VIS_CW;
    const int o = own[r + 1][c + 1];
    bool f = false;
    if (o >= 0) {
      const int up = own[r][c + 1], dn = own[r + 2][c + 1], lf = own[r + 1][c], rt = own[r + 1][c + 2];
      f = (up != -2 && up != o) || (dn != -2 && dn != o) || (lf != -2 && lf != o) || (rt != -2 && rt != o);
    }
    cont[r][c] = f ? 1 : 0;
  }
  __syncthreads();
  const int row = threadIdx.x >> 4, col = (threadIdx.x & 15) * 4;          // 16 lanes of 4 pixels per tile row
  const int y = y0 + row, x = x0 + col;
  if (y >= H || x >= W) return;
  const size_t pix = (size_t)b * plane + (size_t)y * W + x;
  // wide: W % 4 == 0 and 4-byte aligned operands (the entry point decides); then x + 3 < W and 3 pix is a multiple of 4.
  // The four pixels are three words in registers on both paths (every index below is a constant after unrolling: no scratch).
  const int nbytes = (W - x < 4 ? W - x : 4) * 3;
  unsigned iw[3] = {0u, 0u, 0u}, sw[3] = {0u, 0u, 0u}, ow[3] = {0u, 0u, 0u};
  if (wide) {
    const unsigned *src = reinterpret_cast<const unsigned *>(image + pix * 3);
    iw[0] = src[0];
    iw[1] = src[1];
    iw[2] = src[2];
    if (shade) {
      const unsigned *s2 = reinterpret_cast<const unsigned *>(shade + pix * 3);
      sw[0] = s2[0];
      sw[1] = s2[1];
      sw[2] = s2[2];
    }
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      if (k < nbytes) {
        iw[k >> 2] |= (unsigned)image[pix * 3 + k] << (8 * (k & 3));
        if (shade) sw[k >> 2] |= (unsigned)shade[pix * 3 + k] << (8 * (k & 3));
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {                                            // a pixel past the row's end is computed and not stored
    unsigned ch[3], sc[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      ch[c] = (iw[(3 * k + c) >> 2] >> (8 * ((3 * k + c) & 3))) & 255u;
      sc[c] = (sw[(3 * k + c) >> 2] >> (8 * ((3 * k + c) & 3))) & 255u;
    }
    if (gray) ch[0] = ch[1] = ch[2] = vis_gray(ch[0], ch[1], ch[2]);
    const int o = own[row + VIS_HALO][col + k + VIS_HALO];
    if (o >= 0) {
      if (!shade) {
        const uint8_t *c = colors + (size_t)(o < n_ids ? o : n_ids - 1) * 3;
        sc[0] = c[0];
        sc[1] = c[1];
        sc[2] = c[2];
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) ch[c] = vis_blend(sc[c], ch[c], (unsigned)alpha);
    }
    bool edge = false;
    for (int j = 0; j < w; ++j)
      for (int i = 0; i < w; ++i) edge = edge || cont[row + 3 - j][col + k + 3 - i];     // outside the image: own = -2, flag 0
    if (edge) {
      ch[0] = edge_rgb & 255u;
      ch[1] = (edge_rgb >> 8) & 255u;
      ch[2] = (edge_rgb >> 16) & 255u;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) ow[(3 * k + c) >> 2] |= ch[c] << (8 * ((3 * k + c) & 3));
  }
  if (wide) {
    unsigned *dst = reinterpret_cast<unsigned *>(out + pix * 3);
    dst[0] = ow[0];
    dst[1] = ow[1];
    dst[2] = ow[2];
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k)
      if (k < nbytes) out[pix * 3 + k] = (uint8_t)(ow[k >> 2] >> (8 * (k & 3)));
  }
}

__device__ __forceinline__ int vis_pixel(float f) {
  const float g = floorf(f);
  return g < (float)VIS_CLAMP_LO ? VIS_CLAMP_LO : g > (float)VIS_CLAMP_HI ? VIS_CLAMP_HI : (int)g;
}

__device__ __forceinline__ bool vis_finite(float f) { return (__float_as_uint(f) & 0x7f800000u) != 0x7f800000u; }

__global__ __launch_bounds__(VIS_THREADS) void vis_project_kernel(const float *__restrict__ points, const int *__restrict__ inst,
                                                                  const float *__restrict__ R, const float *__restrict__ t,
                                                                  const float *__restrict__ cams, long M, int N, float znear,
                                                                  int *__restrict__ xy, uint8_t *__restrict__ valid) {
  const long m = (long)blockIdx.x * VIS_THREADS + threadIdx.x;
  if (m >= M) return;
  const int n = inst[m];
  int px = 0, py = 0;
  bool ok = false;
  if (n >= 0 && n < N) {
    const float x = points[m * 3 + 0], y = points[m * 3 + 1], z = points[m * 3 + 2];
    const float *r = R + (size_t)n * 9, *tt = t + (size_t)n * 3, *k = cams + (size_t)n * 4;
    const float xc = ((r[0] * x + r[1] * y) + r[2] * z) + tt[0];
    const float yc = ((r[3] * x + r[4] * y) + r[5] * z) + tt[1];
    const float zc = ((r[6] * x + r[7] * y) + r[8] * z) + tt[2];
    const float u = (k[0] * xc) / zc + k[2];
    const float v = (k[1] * yc) / zc + k[3];
    ok = zc >= znear && vis_finite(u) && vis_finite(v);
    if (ok) {
      px = vis_pixel(u);
      py = vis_pixel(v);
    }
  }
  xy[m * 2 + 0] = px;
  xy[m * 2 + 1] = py;
  valid[m] = ok ? 1 : 0;
}

struct VisPrim {
  int x0, y0, x1, y1, size;
  unsigned rgb;
};

__device__ __forceinline__ bool vis_in_clamp(int v) { return v >= VIS_CLAMP_LO && v <= VIS_CLAMP_HI; }

__device__ __forceinline__ bool vis_covers(const VisPrim &q, int x, int y) {
  const long dx = (long)q.x1 - q.x0, dy = (long)q.y1 - q.y0;
  const long ax = (long)x - q.x0, ay = (long)y - q.y0;
  const long L = dx * dx + dy * dy, uu = ax * dx + ay * dy, s2 = (long)q.size * q.size;
  if (L == 0 || uu <= 0) return 4 * (ax * ax + ay * ay) <= s2;
  if (uu >= L) {
    const long bx = (long)x - q.x1, by = (long)y - q.y1;
    return 4 * (bx * bx + by * by) <= s2;
  }
  const long cr = ax * dy - ay * dx;
  return 4 * cr * cr <= s2 * L;
}

__global__ __launch_bounds__(VIS_THREADS) void vis_draw_kernel(const int *__restrict__ prims, const long *__restrict__ frame_start,
                                                               long P, int H, int W, int tiles_x, int tiles_y,
                                                               uint8_t *__restrict__ image) {
  __shared__ VisPrim hits[S6D_VIS_DRAW_CHUNK];
  __shared__ unsigned wave_tot[VIS_THREADS / kWave];
  const int tiles = tiles_x * tiles_y;
  const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int X0 = tx * VIS_DW, Y0 = ty * VIS_DH;
  const int X1 = (X0 + VIS_DW < W ? X0 + VIS_DW : W) - 1, Y1 = (Y0 + VIS_DH < H ? Y0 + VIS_DH : H) - 1;      // inclusive
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x = X0 + (threadIdx.x & (VIS_DW - 1)), y = Y0 + threadIdx.x / VIS_DW;
  const bool inside = x < W && y < H;
  long k0 = frame_start[b], k1 = frame_start[b + 1];                  // clamped to the list: nothing is read outside prims (P,8)
  k0 = k0 < 0 ? 0 : k0;
  k1 = k1 > P ? P : k1;
  bool painted = false;
  unsigned rgb = 0;
  for (long c0 = k0; c0 < k1; c0 += S6D_VIS_DRAW_CHUNK) {
    const long k = c0 + threadIdx.x;
    bool hit = false;
    VisPrim q = {0, 0, 0, 0, 0, 0u};
    if (k < k1) {
      const int *e = prims + k * 8;
      q.x0 = e[1];
      q.y0 = e[2];
      q.x1 = e[3];
      q.y1 = e[4];
      q.size = e[5];
      q.rgb = (unsigned)e[6];
      const bool ok = e[0] == b && e[7] != 0 && q.size >= 0 && q.size <= 64 && vis_in_clamp(q.x0) && vis_in_clamp(q.y0) &&
                      vis_in_clamp(q.x1) && vis_in_clamp(q.y1);
      const int r = (q.size + 1) >> 1;
      const int lox = (q.x0 < q.x1 ? q.x0 : q.x1) - r, hix = (q.x0 > q.x1 ? q.x0 : q.x1) + r;
      const int loy = (q.y0 < q.y1 ? q.y0 : q.y1) - r, hiy = (q.y0 > q.y1 ? q.y0 : q.y1) + r;
      hit = ok && lox <= X1 && hix >= X0 && loy <= Y1 && hiy >= Y0;
    }
    // the hits in list order: rank inside the wave by the ballot, the waves before it by their totals
    const unsigned long long bal = __ballot(hit);
    const int rank = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wave_tot[wave] = (unsigned)__popcll(bal);
    __syncthreads();
    unsigned off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < VIS_THREADS / kWave; ++w) {
      if (w < wave) off += wave_tot[w];
      tot += wave_tot[w];
    }
    if (hit) hits[off + rank] = q;
    __syncthreads();
    if (inside) {
      for (unsigned i = 0; i < tot; ++i) {
        const VisPrim h = hits[i];                                       // one address for the wave: a broadcast
        if (vis_covers(h, x, y)) {
          painted = true;
          rgb = h.rgb;
        }
      }
    }
    __syncthreads();                                                     // the readers are done before the next chunk's writers
  }
  if (inside && painted) {
    uint8_t *o = image + ((size_t)b * H * W + (size_t)y * W + x) * 3;
    o[0] = (uint8_t)(rgb & 255u);
    o[1] = (uint8_t)((rgb >> 8) & 255u);
    o[2] = (uint8_t)((rgb >> 16) & 255u);
  }
}

static int vis_size_status(int B, int H, int W) {
  if (B < 0 || H < 1 || W < 1) return S6D_EINVAL;
  if (H > VIS_MAX_HW || W > VIS_MAX_HW) return S6D_EUNSUPPORTED;
  return S6D_OK;
}

}  // namespace s6d

using namespace s6d;

extern "C" int s6d_vis_owner_from_masks(const uint64_t *packed, const int32_t *order, const long *frame_start, int B, int N, long K, int H,
                                        int W, int32_t *owner, void *stream) {
  const int rc = vis_size_status(B, H, W);
  if (rc != S6D_OK) return rc;
  if (N < 0 || K < 0 || K > N) return S6D_EINVAL;
  if (!frame_start || !owner || (K > 0 && (!packed || !order))) return S6D_EINVAL;
  const long plane = (long)H * W, blocks = (plane + VIS_THREADS - 1) / VIS_THREADS;
  if ((long)B * blocks > 0x7fffffffL) return S6D_EUNSUPPORTED;
  if (B == 0) return S6D_OK;
  hipLaunchKernelGGL(vis_owner_kernel, dim3((unsigned)(B * blocks)), dim3(VIS_THREADS), 0, as_stream(stream),
                     reinterpret_cast<const unsigned long long *>(packed), order, frame_start, N, K, plane, (plane + 63) / 64, (int)blocks,
                     owner);
  return launch_status();
}

extern "C" int s6d_vis_merge_layers(const float *depth, const uint8_t *rgb, const int32_t *frame, int T, int first, int B, int H, int W,
                                    float *zbuf, int32_t *owner, uint8_t *shade, void *stream) {
  const int rc = vis_size_status(B, H, W);
  if (rc != S6D_OK) return rc;
  if (T < 0 || first < 0 || (long)first + T > 0x7fffffffL) return S6D_EINVAL;
  if (!depth || !rgb || !frame || !zbuf || !owner || !shade) return S6D_EINVAL;
  const long plane = (long)H * W, blocks = (plane + VIS_THREADS - 1) / VIS_THREADS;
  if ((long)B * blocks > 0x7fffffffL) return S6D_EUNSUPPORTED;
  if (B == 0 || T == 0) return S6D_OK;
  hipLaunchKernelGGL(vis_merge_kernel, dim3((unsigned)(B * blocks)), dim3(VIS_THREADS), 0, as_stream(stream), depth, rgb, frame, T,
                     first, plane, (int)blocks, zbuf, owner, shade);
  return launch_status();
}

extern "C" int s6d_vis_paint_u8(const uint8_t *image, const int32_t *owner, const uint8_t *colors, const uint8_t *shade, int n_ids, int B,
                                int H, int W, int gray, int alpha, int edge_width, int edge_r, int edge_g, int edge_b, uint8_t *out,
                                void *stream) {
  const int rc = vis_size_status(B, H, W);
  if (rc != S6D_OK) return rc;
  if (alpha < 0 || alpha > 256 || edge_width < 0 || edge_width > VIS_HALO || (gray != 0 && gray != 1)) return S6D_EINVAL;
  if (edge_r < 0 || edge_r > 255 || edge_g < 0 || edge_g > 255 || edge_b < 0 || edge_b > 255) return S6D_EINVAL;
  if (!image || !owner || !out || (!shade && (!colors || n_ids < 1))) return S6D_EINVAL;
  const long tiles_x = (W + VIS_TW - 1) / VIS_TW, tiles_y = (H + VIS_TH - 1) / VIS_TH;
  if ((long)B * tiles_x * tiles_y > 0x7fffffffL) return S6D_EUNSUPPORTED;
  if (B == 0) return S6D_OK;
  const uintptr_t bits = (uintptr_t)image | (uintptr_t)out | (uintptr_t)shade;
  const int wide = (W & 3) == 0 && (bits & 3) == 0;
  hipLaunchKernelGGL(vis_paint_kernel, dim3((unsigned)(B * tiles_x * tiles_y)), dim3(VIS_THREADS), 0, as_stream(stream), image, owner,
                     colors, shade, n_ids, H, W, (int)tiles_x, (int)tiles_y, gray, alpha, edge_width,
                     (unsigned)edge_r | ((unsigned)edge_g << 8) | ((unsigned)edge_b << 16), wide, out);
  return launch_status();
}

extern "C" int s6d_vis_project_f32(const float *points, const int32_t *inst, const float *R, const float *t, const float *cams, long M,
                                   int N, float znear, int32_t *xy, uint8_t *valid, void *stream) {
  if (M < 0 || N < 0 || !(znear == znear)) return S6D_EINVAL;
  const long blocks = (M + VIS_THREADS - 1) / VIS_THREADS;
  if (blocks > 0x7fffffffL) return S6D_EUNSUPPORTED;
  if (!points || !inst || !xy || !valid || (N > 0 && (!R || !t || !cams))) return S6D_EINVAL;
  if (M == 0) return S6D_OK;
  hipLaunchKernelGGL(vis_project_kernel, dim3((unsigned)blocks), dim3(VIS_THREADS), 0, as_stream(stream), points, inst, R, t, cams, M, N,
                     znear, xy, valid);
  return launch_status();
}

extern "C" int s6d_vis_draw_u8(const int32_t *prims, const long *frame_start, int B, long P, int H, int W, uint8_t *image, void *stream) {
  const int rc = vis_size_status(B, H, W);
  if (rc != S6D_OK) return rc;
  if (P < 0) return S6D_EINVAL;
  if (!frame_start || !image || (P > 0 && !prims)) return S6D_EINVAL;
  const long tiles_x = (W + VIS_DW - 1) / VIS_DW, tiles_y = (H + VIS_DH - 1) / VIS_DH;
  if ((long)B * tiles_x * tiles_y > 0x7fffffffL) return S6D_EUNSUPPORTED;
  if (B == 0 || P == 0) return S6D_OK;
  hipLaunchKernelGGL(vis_draw_kernel, dim3((unsigned)(B * tiles_x * tiles_y)), dim3(VIS_THREADS), 0, as_stream(stream), prims, frame_start,
                     P, H, W, (int)tiles_x, (int)tiles_y, image);
  return launch_status();
}
