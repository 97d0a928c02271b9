// Feature similarity of the PEM matching heads (gfx950): atten = normalize(f1) . normalize(f2)^T / temp in one launch, with a fixed
// accumulation order per instance (no library GEMM whose kernel -- and with it the last bit of atten -- follows the batch size).
//
// Reference: compute_feature_similarity, Pose_Estimation_Model/utils/model_utils.py:114-136, sim_type 'cosine', normalize_feat=True:
//   F.normalize(f1, p=2, dim=2) @ F.normalize(f2, p=2, dim=2).transpose(1, 2) / temp
//
// cosine_sim_kernel, grid = (32-row panels of f1) x B flattened, 512 threads = 8 waves:
//   * the workgroup normalises its panel of f1 rows into LDS once, then streams f2 through LDS in chunks of `nb` rows (64, or 32
//     where C > 424 would not fit the 160 KiB), normalising each chunk as it arrives: no normalised copy ever reaches HBM;
//   * wave w owns the 16 x 16 tile (row tile w & 1, column tile w >> 1) of the 32 x nb block: C / 4 exact-fp32 matrix instructions
//     (v_mfma_f32_16x16x4_f32) whose operands are single floats read from LDS -- lane l supplies k = k0 + (l >> 4);
//   * rows past M1 / M2 are zero rows in LDS (zero-filled fragments), the stores are guarded.
// LDS rows are C + 2 floats apart: with C % 16 == 0 the 32 lanes of a ds_read_b32 group (16 rows x 2 values of k) fall on 32
// different banks.
//
// Fixed arithmetic (every operation below is its own IEEE float32 operation: contraction is off in the functions that hold them,
// the library is built without fast-math, sqrtf and `/` are the correctly rounded forms):
//   ss   lane l of the wave that normalises a row holds x[4l .. 4l+3] and, for C > 256, x[256+4l .. 256+4l+3] (zeros past C);
//        its partial is ((((x0^2 + x1^2) + x2^2) + x3^2) + ...) in ascending k, and the 64 partials are summed by the xor butterfly
//        32, 16, 8, 4, 2, 1 -- the order depends on C alone: not on B, the panel, the chunk or the side (f1 / f2) the row is on
//   n    max(sqrtf(ss), 1e-12f)                                         (F.normalize's eps)
//   x^   x / n                                                          (a division, not a product with a reciprocal)
//   dot  acc = fma(x^1[k], x^2[k], acc) for k = 0 .. C-1 ascending, acc = 0 at the start: the matrix instruction is an fma chain
//        over its four k, and the instructions follow each other in ascending k0
//   out  dot / temp                                                     (a division)
// Consequences: an all-zero row gives an exactly zero row / column; a row whose squares overflow (ss = inf) is divided by inf and
// gives zeros too, as torch's statement does; a tiny row (sqrt(ss) < 1e-12, whether or not its squares are flushed) is divided by
// 1e-12f; instance b of a batch has the bits it has alone; similarity(f2, f1) is the transpose of similarity(f1, f2) bit for bit
// (the same terms in the same order, the products commute).
#include "s6d_common.h"
#include "s6d_mem.h"

namespace s6d {


constexpr int SIM_THREADS = 512;
constexpr int SIM_WAVES = SIM_THREADS / 64;
constexpr int SIM_ROWS = 32;                                             // f1 rows per workgroup (two row tiles)
constexpr int SIM_MAX_C = 512;
constexpr int SIM_LDS_MAX = 160 * 1024;

// One row of C floats (src == nullptr: a row past the end) normalised into LDS by one wave; dst is 8-byte aligned.
__device__ __forceinline__ void sim_normalise_row(const float *__restrict__ src, float *dst, int C, int lane) {
#pragma clang fp contract(off)
  const int k0 = lane * 4, k1 = 256 + lane * 4;
  float4 u = make_float4(0.f, 0.f, 0.f, 0.f), v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (src != nullptr && k0 < C) u = *reinterpret_cast<const float4 *>(src + k0);
  if (src != nullptr && k1 < C) v = *reinterpret_cast<const float4 *>(src + k1);
  float ss = ((u.x * u.x + u.y * u.y) + u.z * u.z) + u.w * u.w;
  ss = (((ss + v.x * v.x) + v.y * v.y) + v.z * v.z) + v.w * v.w;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss = ss + __shfl_xor(ss, o);
  const float n = fmaxf(sqrtf(ss), 1e-12f);
  if (k0 < C) {
    *reinterpret_cast<float2 *>(dst + k0) = make_float2(u.x / n, u.y / n);
    *reinterpret_cast<float2 *>(dst + k0 + 2) = make_float2(u.z / n, u.w / n);
  }
  if (k1 < C) {
    *reinterpret_cast<float2 *>(dst + k1) = make_float2(v.x / n, v.y / n);
    *reinterpret_cast<float2 *>(dst + k1 + 2) = make_float2(v.z / n, v.w / n);
  }
}

__device__ __forceinline__ float sim_div(float a, float b) {
#pragma clang fp contract(off)
  return a / b;
}

__global__ __launch_bounds__(SIM_THREADS) void cosine_sim_kernel(const float *__restrict__ f1, const float *__restrict__ f2, int M1,
                                                                int M2, int C, int nb, int panels, float temp,
                                                                float *__restrict__ atten) {
  S6D_DYN_LDS(smem);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int b = blockIdx.x / panels, r0 = (blockIdx.x % panels) * SIM_ROWS;
  const int S = C + 2;
  float *As = reinterpret_cast<float *>(smem);                           // [SIM_ROWS][S]
  float *Bs = As + SIM_ROWS * S;                                         // [nb][S]
  const float *F1 = f1 + (size_t)b * M1 * C, *F2 = f2 + (size_t)b * M2 * C;
  float *A = atten + (size_t)b * M1 * M2;

  for (int r = wave; r < SIM_ROWS; r += SIM_WAVES)
    sim_normalise_row(r0 + r < M1 ? F1 + (size_t)(r0 + r) * C : nullptr, As + r * S, C, lane);

  const int c = lane & 15, g = lane >> 4;
  const int rt = wave & 1, ct = wave >> 1;                               // this wave's tile of the 32 x nb block
  const bool has_tile = ct * 16 < nb;
  for (int j0 = 0; j0 < M2; j0 += nb) {
    __syncthreads();                                                     // the previous chunk's tiles have been read
    for (int r = wave; r < nb; r += SIM_WAVES)
      sim_normalise_row(j0 + r < M2 ? F2 + (size_t)(j0 + r) * C : nullptr, Bs + r * S, C, lane);
    __syncthreads();
    if (!has_tile || j0 + ct * 16 >= M2 || r0 + rt * 16 >= M1) continue;   // (wave-uniform) nothing of this tile is stored
    const float *ap = As + (rt * 16 + c) * S + g, *bp = Bs + (ct * 16 + c) * S + g;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    int k = 0;
    for (; k + 32 <= C; k += 32) {                                       // eight instructions' operands are read ahead of the first
      float a[8], bv[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        a[e] = ap[k + 4 * e];
        bv[e] = bp[k + 4 * e];
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], bv[e], acc, 0, 0, 0);
    }
    for (; k < C; k += 4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[k], bp[k], acc, 0, 0, 0);
    const int col = j0 + ct * 16 + c;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = r0 + rt * 16 + g * 4 + r;
      if (row < M1 && col < M2) A[(size_t)row * M2 + col] = sim_div(acc[r], temp);
    }
  }
}

}  // namespace s6d

using namespace s6d;

extern "C" int s6d_cosine_similarity_f32(const float *f1, const float *f2, int B, int M1, int M2, int C, float temp, float *atten,
                                         void *stream) {
  if (B < 0 || M1 <= 0 || M2 <= 0 || C <= 0 || !(temp > 0.f && temp <= 3.402823466e+38f)) return S6D_EINVAL;
  if ((C % 4) != 0 || C > SIM_MAX_C) return S6D_EUNSUPPORTED;
  const long panels = ((long)M1 + SIM_ROWS - 1) / SIM_ROWS;
  if (panels * (long)B > 0x7fffffffL) return S6D_EUNSUPPORTED;
  if (B == 0) return S6D_OK;
  if (!f1 || !f2 || !atten) return S6D_EINVAL;
  if (((uintptr_t)f1 | (uintptr_t)f2) & 15) return S6D_EINVAL;          // rows are read as float4
  const size_t row_bytes = (size_t)(C + 2) * 4;
  const int nb = (SIM_ROWS + 64) * row_bytes <= (size_t)SIM_LDS_MAX ? 64 : 32;
  const size_t lds = (SIM_ROWS + nb) * row_bytes;
  (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&cosine_sim_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(cosine_sim_kernel, dim3((unsigned)(panels * B)), dim3(SIM_THREADS), lds, as_stream(stream), f1, f2, M1, M2, C, nb,
                     (int)panels, temp, atten);
  return launch_status();
}
