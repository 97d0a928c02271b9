// hipcc-flags: -ffp-contract=off
// Pose refinement against the measured depth on the device (gfx950): one Gauss-Newton step of projective point-to-plane ICP for T
// instances of one mesh.  SAM-6D has no refinement, so nothing here restates a reference: the step is DEFINED
// below, operation by operation, and the tests pin the kernels to an independent restatement of this header (tests/refine_ref.py).
//
// Inputs per instance t: xyz[t] (H,W,3) f32 model coordinates and face[t] (H,W) i32 of `s6d_raster_views_f32` at the current pose,
// the pose P[t] (4,4) f32 object -> camera (R its upper 3 x 3, tr its last column, model units), the mesh (vertices (V,3) f32, faces
// (F,3) i32), the measured depth depth_obs[obs_index[t]] (H,W) f32, optionally mask[t] (H,W) u8, and fx fy cx cy depth_unit max_dist
// min_cos as floats.
//
// Fixed arithmetic: float64 formed from the float32 inputs, every operation rounded on its own (contraction is off for this file,
// `/` and sqrt are the correctly rounded forms); a three-term sum is (a + b) + c.
//
// refine_partial_kernel, at pixel (u, v), p = v W + u:
//   f = face.  The pixel takes part only if 0 <= f < F, the three vertex indices of face f lie in [0, V), the mask (when given) is
//       not 0, and Zo = (double)depth * (double)depth_unit satisfies Zo > 0 (NaN fails).
//   q = ((((double)u - cx) / fx) Zo, (((double)v - cy) / fy) Zo, Zo).
//   x = xyz at the pixel;  p_i = ((R_i0 x_0 + R_i1 x_1) + R_i2 x_2) + tr_i.
//   a = v1 - v0, b = v2 - v0 of face f;  m = a x b = (a_1 b_2 - a_2 b_1, a_2 b_0 - a_0 b_2, a_0 b_1 - a_1 b_0);
//       mm = (m_0 m_0 + m_1 m_1) + m_2 m_2;  mm == 0 rejects;  w = m / sqrt(mm);  n_i = (R_i0 w_0 + R_i1 w_1) + R_i2 w_2;
//       np = (n_0 p_0 + n_1 p_1) + n_2 p_2;  if np > 0 then n = -n and np = -np (the visible side faces the camera at the origin).
//   grazing   reject unless np np >= (min_cos min_cos) pp,  pp = (p_0 p_0 + p_1 p_1) + p_2 p_2.
//   outliers  d = q - p;  reject unless (d_0 d_0 + d_1 d_1) + d_2 d_2 <= max_dist max_dist.   (Both tests are written so NaN rejects.)
//   r = (n_0 d_0 + n_1 d_1) + n_2 d_2;  J = (p x n, n) = (p_1 n_2 - p_2 n_1, p_2 n_0 - p_0 n_2, p_0 n_1 - p_1 n_0, n_0, n_1, n_2).
//   The pixel adds the 28 terms  J_i J_j (i <= j, row-major: 00 01 .. 05 11 12 .. 55),  J_i r (i = 0 .. 5),  r r  and 1 to a count.
//   reduction  a workgroup of 256 lanes owns the S6D_RF_CHUNK consecutive row-major pixels [c CHUNK, (c + 1) CHUNK) of ONE instance;
//              lane l visits p = c CHUNK + l, + 256, ... and adds in visiting order from +0; the wave reduces every term by the xor
//              butterfly x += shuffle_xor(x, o), o = 32, 16, 8, 4, 2, 1; wave 0 .. 3 are added in wave order ((w0 + w1) + w2) + w3
//              through LDS; the 28 partial sums and the count of (instance, chunk) go to the workspace with plain vector stores.
//              (A wave or a workgroup without a correspondence writes +0 without the shuffles: the same bits.)
//              An obs_index outside [0, M) gives every chunk of the instance zeros (the wrapper refuses it on the host).
// refine_fold_kernel: one workgroup per instance, lane k < 28 adds the partials of term k in chunk order from +0; lane 28 the counts.
//              No floating-point atomic anywhere: an instance has the same bits alone and in a batch, under any scheduling.
//
// refine_update_kernel, one workgroup per instance (its lane 0; the system is 6 x 6), A the symmetric matrix of the 21 sums, b the
// 6 sums of J r, rr the last, lambda = (double)damping:
//   status 3  if one of the 28 sums or of the 12 entries of the pose's upper three rows is not finite;
//   status 1  else if count < min_count;
//   scaling   d_i = sqrt(A_ii);  M_ij = A_ij / (d_i d_j) for i != j, 0 where d_i d_j == 0;  M_ii = 1 + lambda (also where A_ii = 0);
//             c_i = b_i / d_i, 0 where d_i == 0.   (Jacobi scaling S = diag(A_ii^-1/2): M = S A S + lambda I, c = S b.)
//   Cholesky  M = L L^T, column by column j = 0 .. 5:  s = M_jj;  s = s - L_jk L_jk for k = 0 .. j-1;  status 2 unless s >= min_pivot;
//             L_jj = sqrt(s);  for i = j+1 .. 5:  s = M_ij;  s = s - L_ik L_jk for k = 0 .. j-1;  L_ij = s / L_jj.
//   solve     z_i = (c_i - sum_k<i L_ik z_k) / L_ii for i = 0 .. 5,  y_i = (z_i - sum_k>i L_ki y_k) / L_ii for i = 5 .. 0, the
//             subtractions one at a time in ascending k;  xi_i = y_i / d_i (0 where d_i == 0) = (omega, v).
//   Cayley    h = omega 0.5;  hh = (h_0 h_0 + h_1 h_1) + h_2 h_2;  e = 1 + hh;  g = 1 - hh;  with  xy = 2 (h_0 h_1), ..., x2 = 2 h_0:
//             dR = [ (g + 2 (h_0 h_0)) / e   (xy - z2) / e           (xz + y2) / e
//                    (xy + z2) / e           (g + 2 (h_1 h_1)) / e   (yz - x2) / e
//                    (xz - y2) / e           (yz + x2) / e           (g + 2 (h_2 h_2)) / e ]  = (I - [h]x)^-1 (I + [h]x):
//             a rotation by 2 atan |h| about h, with + x / sqrt only: the same bits on every platform.
//   update    R'_ij = (float)((dR_i0 R_0j + dR_i1 R_1j) + dR_i2 R_2j),  tr'_i = (float)((((dR_i0 tr_0 + dR_i1 tr_1) + dR_i2 tr_2)) + v_i);
//             the fourth row is copied.  status 3 if an entry of R' or tr' is not finite.
//   Any non-zero status copies the 16 input floats through bit for bit.   rms = sqrt(rr / (double)count) where the sums are finite
//   and count > 0, else 0.
#include "s6d_common.h"

namespace s6d {

#pragma clang fp contract(off)   // the stated float64 operations, one rounding each

constexpr int RF_THREADS = 256;
constexpr int RF_WAVES = RF_THREADS / kWave;
constexpr int RF_TERMS = 28;
constexpr int RF_CHUNK = S6D_RF_CHUNK;                                   // pixels of one workgroup
constexpr int RF_VISITS = RF_CHUNK / RF_THREADS;
static_assert(RF_CHUNK % RF_THREADS == 0, "a lane visits a whole number of pixels");

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ bool rf_finite(double x) { return x - x == 0.0; }

// Work per lane is uneven: most pixels fail the face / depth predicate.  Neighbouring pixels sit in neighbouring lanes, so a wave is
// either (nearly) full of object pixels or empty, and an empty wave takes no part of the float64 path; the cheap operands (face,
// depth, mask: 9 of the 21 bytes) of a lane's RF_VISITS pixels are requested before any of them is used, xyz only where they pass.
__global__ __launch_bounds__(RF_THREADS) void refine_partial_kernel(
    const float *__restrict__ xyz, const int *__restrict__ face, const float *__restrict__ depth_obs, const int *__restrict__ obs_index,
    const uint8_t *__restrict__ mask, const float *__restrict__ vertices, const int *__restrict__ faces, const float *__restrict__ poses,
    int V, int F, int M, int W, long plane, int chunks, float fx32, float fy32, float cx32, float cy32, float unit32, float max_dist32,
    float min_cos32, double *__restrict__ part, int *__restrict__ pcount) {
  __shared__ double red[RF_TERMS][RF_WAVES];
  __shared__ int redc[RF_WAVES];
  const int t = blockIdx.x / chunks, chunk = blockIdx.x - t * chunks;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ti = obs_index[t];
  const bool live = ti >= 0 && ti < M;                                    // wave-uniform: nothing is read out of bounds
  const double fx = fx32, fy = fy32, cx = cx32, cy = cy32, unit = unit32;
  const double md2 = (double)max_dist32 * (double)max_dist32, mc2 = (double)min_cos32 * (double)min_cos32;
  double acc[RF_TERMS];
#pragma unroll
  for (int k = 0; k < RF_TERMS; ++k) acc[k] = 0.0;
  int cnt = 0;
  if (live) {
    const float *X = xyz + (size_t)t * plane * 3, *Z = depth_obs + (size_t)ti * plane, *P = poses + (size_t)t * 16;
    const int *FA = face + (size_t)t * plane;
    const uint8_t *MK = mask ? mask + (size_t)t * plane : nullptr;
    const long p0 = (long)chunk * RF_CHUNK + threadIdx.x;
    int fs[RF_VISITS];
    float zs[RF_VISITS];
    int ms[RF_VISITS];
#pragma unroll
    for (int i = 0; i < RF_VISITS; ++i) {
      const long p = p0 + (long)i * RF_THREADS;
      const bool in = p < plane;
      fs[i] = in ? FA[p] : -1;
      zs[i] = in ? Z[p] : 0.f;
      ms[i] = in && MK ? MK[p] : 1;
    }
    double R[9], tr[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) R[i * 3 + j] = P[i * 4 + j];
      tr[i] = P[i * 4 + 3];
    }
#pragma unroll
    for (int i = 0; i < RF_VISITS; ++i) {
      const int f = fs[i];
      const double Zo = (double)zs[i] * unit;
      if (f < 0 || f >= F || ms[i] == 0 || !(Zo > 0.0)) continue;
      const int i0 = faces[(size_t)f * 3 + 0], i1 = faces[(size_t)f * 3 + 1], i2 = faces[(size_t)f * 3 + 2];
      if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) continue;
      const long p = p0 + (long)i * RF_THREADS;
      const int v = (int)(p / W), u = (int)(p - (long)v * W);
      const double q0 = (((double)u - cx) / fx) * Zo, q1 = (((double)v - cy) / fy) * Zo, q2 = Zo;
      const double x0 = X[p * 3 + 0], x1 = X[p * 3 + 1], x2 = X[p * 3 + 2];
      const double c0 = ((R[0] * x0 + R[1] * x1) + R[2] * x2) + tr[0];
      const double c1 = ((R[3] * x0 + R[4] * x1) + R[5] * x2) + tr[1];
      const double c2 = ((R[6] * x0 + R[7] * x1) + R[8] * x2) + tr[2];
      const float *A0 = vertices + (size_t)i0 * 3, *A1 = vertices + (size_t)i1 * 3, *A2 = vertices + (size_t)i2 * 3;
      const double a0 = (double)A1[0] - (double)A0[0], a1 = (double)A1[1] - (double)A0[1], a2 = (double)A1[2] - (double)A0[2];
      const double b0 = (double)A2[0] - (double)A0[0], b1 = (double)A2[1] - (double)A0[1], b2 = (double)A2[2] - (double)A0[2];
      const double m0 = a1 * b2 - a2 * b1, m1 = a2 * b0 - a0 * b2, m2 = a0 * b1 - a1 * b0;
      const double mm = (m0 * m0 + m1 * m1) + m2 * m2;
      if (mm == 0.0) continue;
      const double sm = sqrt(mm);
      const double w0 = m0 / sm, w1 = m1 / sm, w2 = m2 / sm;
      double n0 = (R[0] * w0 + R[1] * w1) + R[2] * w2;
      double n1 = (R[3] * w0 + R[4] * w1) + R[5] * w2;
      double n2 = (R[6] * w0 + R[7] * w1) + R[8] * w2;
      double np = (n0 * c0 + n1 * c1) + n2 * c2;
      if (np > 0.0) {
        n0 = -n0;
        n1 = -n1;
        n2 = -n2;
        np = -np;
      }
      const double pp = (c0 * c0 + c1 * c1) + c2 * c2;
      if (!(np * np >= mc2 * pp)) continue;
      const double d0 = q0 - c0, d1 = q1 - c1, d2 = q2 - c2;
      if (!((d0 * d0 + d1 * d1) + d2 * d2 <= md2)) continue;
      const double r = (n0 * d0 + n1 * d1) + n2 * d2;
      const double J[6] = {c1 * n2 - c2 * n1, c2 * n0 - c0 * n2, c0 * n1 - c1 * n0, n0, n1, n2};
      int k = 0;
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) acc[k++] += J[a] * J[b];
#pragma unroll
      for (int a = 0; a < 6; ++a) acc[21 + a] += J[a] * r;
      acc[27] += r * r;
      cnt += 1;
    }
  }
  const int wcnt = wave_sum_i32(cnt);
  if (wcnt != 0) {                                                       // wave-uniform
#pragma unroll
    for (int k = 0; k < RF_TERMS; ++k) acc[k] = wave_sum_f64(acc[k]);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < RF_TERMS; ++k) red[k][wave] = acc[k];           // +0 from a wave without a correspondence
    redc[wave] = wcnt;
  }
  __syncthreads();
  if (threadIdx.x < RF_TERMS) {
    const int k = threadIdx.x;
    part[(size_t)blockIdx.x * RF_TERMS + k] = ((red[k][0] + red[k][1]) + red[k][2]) + red[k][3];
  } else if (threadIdx.x == RF_TERMS) {
    pcount[blockIdx.x] = ((redc[0] + redc[1]) + redc[2]) + redc[3];
  }
}

__global__ __launch_bounds__(kWave) void refine_fold_kernel(const double *__restrict__ part, const int *__restrict__ pcount, int chunks,
                                                            double *__restrict__ sums, int *__restrict__ count) {
  const int t = blockIdx.x, k = threadIdx.x;
  if (k < RF_TERMS) {
    const double *src = part + (size_t)t * chunks * RF_TERMS + k;
    double s = 0.0;
    int c = 0;
    for (; c + 8 <= chunks; c += 8) {                                    // eight loads in flight, then the additions in chunk order
      double x[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) x[i] = src[(size_t)(c + i) * RF_TERMS];
#pragma unroll
      for (int i = 0; i < 8; ++i) s += x[i];
    }
    for (; c < chunks; ++c) s += src[(size_t)c * RF_TERMS];
    sums[(size_t)t * RF_TERMS + k] = s;
  } else if (k == RF_TERMS) {
    int s = 0;
    for (int c = 0; c < chunks; ++c) s += pcount[(size_t)t * chunks + c];
    count[t] = s;
  }
}

__global__ __launch_bounds__(kWave) void refine_update_kernel(const double *__restrict__ sums, const int *__restrict__ count,
                                                              const float *__restrict__ poses, int min_count, float damping32,
                                                              float min_pivot32, float *__restrict__ poses_out,
                                                              int *__restrict__ status, double *__restrict__ rms) {
  if (threadIdx.x != 0) return;
  const int t = blockIdx.x;
  const double *S = sums + (size_t)t * RF_TERMS;
  const float *P = poses + (size_t)t * 16;
  float *O = poses_out + (size_t)t * 16;
  const int n = count[t];
  float out[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) out[k] = P[k];
  bool finite = true;
#pragma unroll
  for (int k = 0; k < RF_TERMS; ++k) finite = finite && rf_finite(S[k]);
  rms[t] = finite && n > 0 ? sqrt(S[27] / (double)n) : 0.0;
#pragma unroll
  for (int k = 0; k < 12; ++k) finite = finite && rf_finite((double)P[k]);
  int st = !finite ? 3 : n < min_count ? 1 : 0;
  if (st == 0) {                                                         // (every loop unrolls: the 6 x 6 system stays in registers)
    const double lambda = damping32, min_pivot = min_pivot32;
    double A[6][6], d[6], c[6], L[6][6];
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j) A[i][j] = A[j][i] = S[k++];
#pragma unroll
    for (int i = 0; i < 6; ++i) d[i] = sqrt(A[i][i]);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      c[i] = d[i] == 0.0 ? 0.0 : S[21 + i] / d[i];
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        const double dd = d[i] * d[j];
        A[i][j] = i == j ? 1.0 + lambda : dd == 0.0 ? 0.0 : A[i][j] / dd;   // every entry is divided once, by its own d_i d_j
      }
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      double s = A[j][j];
#pragma unroll
      for (int q = 0; q < j; ++q) s = s - L[j][q] * L[j][q];
      if (!(s >= min_pivot)) st = 2;                                     // what follows is computed and thrown away
      L[j][j] = sqrt(s);
#pragma unroll
      for (int i = j + 1; i < 6; ++i) {
        s = A[i][j];
#pragma unroll
        for (int q = 0; q < j; ++q) s = s - L[i][q] * L[j][q];
        L[i][j] = s / L[j][j];
      }
    }
    double z[6], y[6], xi[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double s = c[i];
#pragma unroll
      for (int q = 0; q < i; ++q) s = s - L[i][q] * z[q];
      z[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
      double s = z[i];
#pragma unroll
      for (int q = i + 1; q < 6; ++q) s = s - L[q][i] * y[q];
      y[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) xi[i] = d[i] == 0.0 ? 0.0 : y[i] / d[i];
    const double h0 = xi[0] * 0.5, h1 = xi[1] * 0.5, h2 = xi[2] * 0.5;
    const double hh = (h0 * h0 + h1 * h1) + h2 * h2, e = 1.0 + hh, g = 1.0 - hh;
    const double xy = 2.0 * (h0 * h1), xz = 2.0 * (h0 * h2), yz = 2.0 * (h1 * h2), x2 = 2.0 * h0, y2 = 2.0 * h1, z2 = 2.0 * h2;
    const double dR[3][3] = {{(g + 2.0 * (h0 * h0)) / e, (xy - z2) / e, (xz + y2) / e},
                             {(xy + z2) / e, (g + 2.0 * (h1 * h1)) / e, (yz - x2) / e},
                             {(xz - y2) / e, (yz + x2) / e, (g + 2.0 * (h2 * h2)) / e}};
    float nw[12];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j)
        nw[i * 4 + j] = (float)((dR[i][0] * (double)P[j] + dR[i][1] * (double)P[4 + j]) + dR[i][2] * (double)P[8 + j]);
      nw[i * 4 + 3] = (float)(((dR[i][0] * (double)P[3] + dR[i][1] * (double)P[7]) + dR[i][2] * (double)P[11]) + xi[3 + i]);
    }
#pragma unroll
    for (int q = 0; q < 12; ++q) ok = ok && rf_finite((double)nw[q]);
    if (st == 0 && !ok) st = 3;
    if (st == 0) {
#pragma unroll
      for (int q = 0; q < 12; ++q) out[q] = nw[q];
    }
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) O[k] = out[k];
  status[t] = st;
}

}  // namespace s6d

using namespace s6d;

static long refine_chunks(int H, int W) { return ((long)H * W + RF_CHUNK - 1) / RF_CHUNK; }

extern "C" long s6d_refine_workspace_bytes(int T, int H, int W) {
  if (T < 0 || H < 1 || W < 1) return -1;
  const long plane = (long)H * W, items = (long)T * refine_chunks(H, W);
  if (plane > 0x7fffffffL || items > 0x7fffffffL) return -1;
  return items * RF_TERMS * 8 + (items * 4 + 7) / 8 * 8;
}

extern "C" int s6d_refine_normal_eq_f64(const float *xyz, const int32_t *face, const float *depth_obs, const int32_t *obs_index,
                                        const uint8_t *mask, const float *vertices, const int32_t *faces, const float *poses, int V,
                                        int F, int T, int M, int H, int W, float fx, float fy, float cx, float cy, float depth_unit,
                                        float max_dist, float min_cos, void *workspace, double *sums, int32_t *count, void *stream) {
  if (V < 1 || F < 1 || T < 0 || M < 1 || H < 1 || W < 1) return S6D_EINVAL;
  if (!(fx > 0.f || fx < 0.f) || !(fy > 0.f || fy < 0.f) || !(cx == cx) || !(cy == cy)) return S6D_EINVAL;
  if (!(depth_unit > 0.f) || !(max_dist >= 0.f && max_dist <= 3.0e38f) || !(min_cos >= 0.f && min_cos <= 1.f)) return S6D_EINVAL;
  const long plane = (long)H * W, chunks = refine_chunks(H, W);
  if (plane > 0x7fffffffL || (long)T * chunks > 0x7fffffffL) return S6D_EUNSUPPORTED;
  if (T == 0) return S6D_OK;
  if (!xyz || !face || !depth_obs || !obs_index || !vertices || !faces || !poses || !workspace || !sums || !count) return S6D_EINVAL;
  hipStream_t s = as_stream(stream);
  const long items = (long)T * chunks;
  double *part = static_cast<double *>(workspace);
  int *pcount = reinterpret_cast<int *>(part + items * RF_TERMS);
  hipLaunchKernelGGL(refine_partial_kernel, dim3((unsigned)items), dim3(RF_THREADS), 0, s, xyz, face, depth_obs, obs_index, mask, vertices,
                     faces, poses, V, F, M, W, plane, (int)chunks, fx, fy, cx, cy, depth_unit, max_dist, min_cos, part, pcount);
  const int rc = launch_status();
  if (rc != S6D_OK) return rc;
  hipLaunchKernelGGL(refine_fold_kernel, dim3((unsigned)T), dim3(kWave), 0, s, part, pcount, (int)chunks, sums, count);
  return launch_status();
}

extern "C" int s6d_refine_update_f64(const double *sums, const int32_t *count, const float *poses, int T, int min_count, float damping,
                                     float min_pivot, float *poses_out, int32_t *status, double *rms, void *stream) {
  if (T < 0 || min_count < 1 || !(damping >= 0.f) || !(min_pivot > 0.f) || damping > 3.0e38f || min_pivot > 3.0e38f) return S6D_EINVAL;
  if (T == 0) return S6D_OK;
  if (!sums || !count || !poses || !poses_out || !status || !rms) return S6D_EINVAL;
  hipLaunchKernelGGL(refine_update_kernel, dim3((unsigned)T), dim3(kWave), 0, as_stream(stream), sums, count, poses, min_count, damping,
                     min_pivot, poses_out, status, rms);
  return launch_status();
}
