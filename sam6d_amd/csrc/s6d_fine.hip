// Fine point matching, similarity + soft assignment in one family of kernels (gfx950): the (B, 2049, 2049) similarity
// matrix of the reference is never written.
//
// Reference (Pose_Estimation_Model):
//   model/fine_point_matching.py:75-80    atten = compute_feature_similarity(out_proj(f1), out_proj(f2), 'cosine', temp)
//   utils/model_utils.py:114-136          L2-normalise both feature sets, bmm, / temp           -> (B, M1, M2) f32, 16.8 MB / instance
//   utils/model_utils.py:250-270          compute_fine_Rt head: softmax(dim=2) * softmax(dim=1), row / column arg-max against the
//                                         background row / column, mask, row-normalise (+1e-6), assign @ pts2, row sums as weights
// The reference streams that matrix >= 8 times; round 1 of this repo wrote it once (library bmm) and streamed it 3 times.
//
// Here the matrix exists only as 32 x 32 accumulator tiles.  With e_ij = exp(s_ij), r_i = sum_j e_ij, c_j = sum_i e_ij:
//   p_ij  = (e_ij / r_i)(e_ij / c_j)                               softmax(dim=2) * softmax(dim=1)
//   w2_j  = [argmax_i p_ij > 0]   = [argmax_i e_ij^2 / r_i > 0]    c_j is constant along a column
//   w1_i  = [argmax_j p_ij > 0]   = [argmax_j e_ij^2 / c_j > 0]    r_i is constant along a row
//   wsum_i = w1_i / r_i * sum_{j>=1} e_ij^2 w2_j / c_j,   pred_i = w1_i / r_i * sum_{j>=1} e_ij^2 (w2_j / c_j) pts2_j / (wsum_i + 1e-6)
// so three sweeps over the tile space suffice, each recomputing the tiles on the matrix cores:
//   sweep A  owner = rows i >= 1 of f1, stream = all rows of f2     -> r_i
//   sweep B  owner = rows j >= 1 of f2, stream = all rows of f1     -> c_j, w2_j            (needs r)
//   sweep C  owner = rows i >= 1 of f1, stream = all rows of f2     -> w1_i, wsum_i, pred_i (needs r, c, w2)
// and the background row / column sums r_0, c_0 (one owner each) come from a small kernel pair that repeats the sweeps' arithmetic
// for that one owner (fine_bg_exp_kernel, fine_bg_sum_kernel below: the tie rule needs their bits).
//
// Arithmetic: no max shift is taken, so 1/temp is bounded: S6D_FINE_MATCH_MAX_INV_TEMP = 25 (include/sam6d_hip.h derives it from the arg-max keys e^2 / c; the
// shipped temp = 0.1 gives |s| <= 10 and sums below 2049 e^10).  Labels and weights need fp32-class
// similarities (a bf16 product is off by 3e-2 in s): every normalised row is split x = hi + lo into two bf16 vectors and a tile is
// hi.hi + lo.hi + hi.lo on v_mfma_f32_32x32x16_bf16 (48 MFMAs per 32 x 32 x 256 tile; the dropped lo.lo term is < 2^-16 of
// a product).  log2(e) / temp is folded into the f1 side, so e = v_exp_f32(accumulator).
//
// Structure of a sweep (one 512-thread workgroup per 256 owner rows; at B = 32 that is 256 workgroups = one per CU):
//   * a wave keeps its 32 owner rows as B-operand fragments in registers for the whole sweep (128 VGPRs: 16 k-steps x {hi, lo});
//   * the stream side passes through LDS in tiles of 32 rows x 1 KiB ([hi 512 B | lo 512 B] per row), double buffered, filled by
//     LDS-DMA one tile ahead (a 1-KiB piece = one row; the 16-byte chunk a lane fetches is permuted by the row so that the
//     A-fragment ds_read_b128 of 32 rows x one chunk column is bank-conflict free);
//   * the accumulator layout gives lane <-> owner row, register <-> stream row: every per-owner reduction (sums, arg-max,
//     weighted point) is a per-lane running value with ONE cross-half exchange at the end of the sweep;
//   * per-stream-row quantities (validity, 1/r, 1/c, w2/c, pts2) are staged per tile in LDS and read as broadcasts;
//   * waves 0-3 run [matrix work of tile t, epilogue of tile t], waves 4-7 [epilogue of tile t-1, matrix work of tile t]: the two
//     waves of a SIMD are half an iteration apart, one on the matrix pipe while the other is in its VALU epilogue.
#include "s6d_bf16.h"

namespace s6d {

constexpr int FM_C = 256;                  // feature width (fine_point_matching out_dim)
constexpr int FM_ROWB = FM_C * 4;          // bytes of a split row: hi (C bf16) | lo (C bf16)
constexpr int FM_TILE = 32;                // stream rows per tile
constexpr int FM_OWN = 256;                // owner rows per workgroup (8 waves x 32)
constexpr int FM_TILEB = FM_TILE * FM_ROWB;   // 32 KiB
constexpr int FM_SIDE = 8;                 // floats per stream row in the side table
constexpr int FM_SIDEB = FM_TILE * FM_SIDE * 4;
constexpr int FM_NSIDE = 4;                // side-table ring: tile t's table is read one barrier interval after tile t + 2 is staged
constexpr int FM_LDSB = 2 * FM_TILEB + FM_NSIDE * FM_SIDEB;

S6D_DYN_LDS(fm_smem);

// ---- split: x -> normalise (F.normalize, eps 1e-12) -> * scale -> hi = bf16(x), lo = bf16(x - hi) -------------------------------
// one wave per row; rows >= M (padding up to a whole tile) are zero
__global__ __launch_bounds__(256) void fine_split_kernel(const float *__restrict__ f, int M, int Mp, float scale,
                                                        u16 *__restrict__ xs) {
  const int b = blockIdx.y, row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= Mp) return;
  uint2 hi = make_uint2(0u, 0u), lo = make_uint2(0u, 0u);
  if (row < M) {
    const float4 v = reinterpret_cast<const float4 *>(f + ((size_t)b * M + row) * FM_C)[lane];
    float ss = wave_sum(v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w);
    const float inv = scale / fmaxf(sqrtf(ss), 1e-12f);
    const float x[4] = {v.x * inv, v.y * inv, v.z * inv, v.w * inv};
    u16 h[4], l[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) bf16_split(x[e], h[e], l[e]);
    hi = make_uint2((unsigned)h[0] | ((unsigned)h[1] << 16), (unsigned)h[2] | ((unsigned)h[3] << 16));
    lo = make_uint2((unsigned)l[0] | ((unsigned)l[1] << 16), (unsigned)l[2] | ((unsigned)l[3] << 16));
  }
  u16 *dst = xs + ((size_t)b * Mp + row) * (2 * FM_C);
  reinterpret_cast<uint2 *>(dst)[lane] = hi;
  reinterpret_cast<uint2 *>(dst + FM_C)[lane] = lo;
}

// ---- background owners: r_0 = sum_j e_0j and c_0 = sum_i e_i0 WITH THE ARITHMETIC OF THE SWEEPS -----------------------------------
// A row tied with the background column (a foreground column j whose feature row equals row 0 of f2, so that s_ij = s_i0 for
// every i) is labelled background by the reference: torch.max returns the first index (model_utils.py:264-267).  The tie lives in
// the keys e_ij^2 / c_j, so it survives only if c_0 has the very bits a sweep would give that column: the same matrix
// instructions in the same order per similarity, the same v_exp_f32, and the same order of additions.  (Until round 16 the two
// background sums came from a VALU kernel with its own dot product and eight partial sums: equal columns got sums that
// differed in the last bits once there were more than two tiles of rows, and the tie went to the foreground.)
//   fine_bg_exp_kernel  grid (FM_BGSPLIT, 2, B), which = 0: owner row 0 of xs1 against the rows of xs2, which = 1: the converse.
//                       A wave takes whole stream tiles; its B operand holds the owner row in every column, the A fragments come
//                       straight from global memory at the addresses the sweeps read through LDS; lanes 0 and 32 (column 0 of the
//                       two halves) write e (0 on padding rows) to ev[b][which][stream row].
//   fine_bg_sum_kernel  grid (2, B): lane h in {0, 1} adds the stream rows of accumulator half h in sweep order (tile ascending,
//                       register ascending: rows 8 k + 4 h .. + 3), lane 0 adds the two halves and writes entry 0 of r / c.
constexpr int FM_BGSPLIT = 4;
__global__ __launch_bounds__(512) void fine_bg_exp_kernel(const u16 *__restrict__ xs1, const u16 *__restrict__ xs2, int M1, int M2,
                                                         int Mp1, int Mp2, float *__restrict__ ev, int ldev) {
  const int which = blockIdx.y, b = blockIdx.z, lane = threadIdx.x & 63, half = lane >> 5, col = lane & 31;
  const int wave = blockIdx.x * 8 + (threadIdx.x >> 6);
  const u16 *own = which == 0 ? xs1 + (size_t)b * Mp1 * (2 * FM_C) : xs2 + (size_t)b * Mp2 * (2 * FM_C);
  const u16 *str = which == 0 ? xs2 + (size_t)b * Mp2 * (2 * FM_C) : xs1 + (size_t)b * Mp1 * (2 * FM_C);
  const int n = which == 0 ? M2 : M1, ntile = (which == 0 ? Mp2 : Mp1) / FM_TILE;
  float *E = ev + ((size_t)b * 2 + which) * ldev;
  bf16x8 bh[16], bl[16];
#pragma unroll
  for (int ks = 0; ks < 16; ++ks) {
    bh[ks] = *reinterpret_cast<const bf16x8 *>(own + 16 * ks + 8 * half);
    bl[ks] = *reinterpret_cast<const bf16x8 *>(own + FM_C + 16 * ks + 8 * half);
  }
  for (int t = wave; t < ntile; t += 8 * FM_BGSPLIT) {
    const u16 *row = str + (size_t)(t * FM_TILE + col) * (2 * FM_C);
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {                                 // the order of tile_mfma below
      const bf16x8 ah = *reinterpret_cast<const bf16x8 *>(row + 16 * ks + 8 * half);
      const bf16x8 al = *reinterpret_cast<const bf16x8 *>(row + FM_C + 16 * ks + 8 * half);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh[ks], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh[ks], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl[ks], acc, 0, 0, 0);
    }
    if (col == 0) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int j = t * FM_TILE + (e & 3) + 8 * (e >> 2) + 4 * half;
        E[j] = j < n ? __builtin_amdgcn_exp2f(acc[e]) : 0.f;
      }
    }
  }
}

__global__ __launch_bounds__(64) void fine_bg_sum_kernel(const float *__restrict__ ev, int ldev, int Mp1, int Mp2, float *__restrict__ r,
                                                        float *__restrict__ c) {
  const int which = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const int ntile = (which == 0 ? Mp2 : Mp1) / FM_TILE;
  const float *E = ev + ((size_t)b * 2 + which) * ldev + 4 * (lane & 1);
  float s = 0.f;
  if (lane < 2) {
#pragma unroll 2
    for (int t = 0; t < ntile; ++t) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float4 v = *reinterpret_cast<const float4 *>(E + t * FM_TILE + 8 * k);
        s += v.x;
        s += v.y;
        s += v.z;
        s += v.w;
      }
    }
  }
  s += __shfl_xor(s, 1);
  if (lane == 0) (which == 0 ? r + (size_t)b * Mp1 : c + (size_t)b * Mp2)[0] = s;
}

struct FineParams {
  const u16 *own;       // (B, Mpo, 512) split rows of the owner side
  const u16 *str;       // (B, Mps, 512) split rows of the stream side
  int Mo, Ms, Mpo, Mps;    // valid rows / padded rows of the two sides
  int B, nblk;             // owner blocks per instance = ceil((Mo - 1) / 256)
  float *r;                // (B, Mp1): row sums (entry 0 from fine_bg_sum_kernel)
  float *c;                // (B, Mp2): column sums (entry 0 likewise)
  float *w2;               // (B, Mp2)
  const float *pts2;       // (B, M2 - 1, 3)
  float *pred, *wsum, *w1; // outputs of sweep C: (B, M1 - 1, 3), (B, M1 - 1), (B, M1 - 1)
  int ldr, ldc;            // row strides of r / c / w2 (= Mp1, Mp2)
};

// side table of stream row j for MODE:  0: {valid}   1: {valid, 1/r_i}   2: {1/c_j, w2_j/c_j, x, y, z}
template <int MODE>
__device__ __forceinline__ void fm_side_row(const FineParams &p, int b, int j, float *out) {
  const bool valid = j < p.Ms;
  out[0] = out[1] = out[2] = out[3] = out[4] = 0.f;
  if (MODE == 0) {
    out[0] = valid ? 1.f : 0.f;
  } else if (MODE == 1) {
    if (valid) {
      const float r = p.r[(size_t)b * p.ldr + j];
      out[0] = 1.f;
      out[1] = 1.0f / r;
    }
  } else {
    if (valid) {
      const float c = p.c[(size_t)b * p.ldc + j];
      const float ic = 1.0f / c;
      out[0] = ic;
      if (j >= 1) {
        const float *q = p.pts2 + ((size_t)b * (p.Ms - 1) + (j - 1)) * 3;
        out[1] = p.w2[(size_t)b * p.ldc + j] * ic;
        out[2] = q[0];
        out[3] = q[1];
        out[4] = q[2];
      }
    }
  }
}

template <int MODE>
__global__ void __launch_bounds__(512, 2) fine_sweep_kernel(FineParams p) {
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, col = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // workgroup -> (instance, owner block).  Workgroup id % 8 is the XCD it runs on (observed dispatch rule, used for speed
  // only): when the shape allows it, the owner blocks of one instance share an XCD, i.e. one L2 copy of their common stream.
  int b, blk;
  {
    const int id = blockIdx.x;
    if ((p.B & 7) == 0 && p.nblk == 8) {
      const int k = id >> 3;
      b = (k >> 3) * 8 + (id & 7);
      blk = k & 7;
    } else {
      b = id / p.nblk;
      blk = id - b * p.nblk;
    }
  }
  const int orow = 1 + blk * FM_OWN + wave * 32 + col;              // this lane's owner row (background row 0 excluded)
  const bool ovalid = orow < p.Mo;
  const int ntile = p.Mps / FM_TILE;

  // ---- owner fragments: B operand of v_mfma_f32_32x32x16_bf16 = column `col`, k = 16 ks + 8 half .. + 7 ----------------------
  bf16x8 bh[16], bl[16];
  {
    const u16 *src = p.own + ((size_t)b * p.Mpo + min(orow, p.Mpo - 1)) * (2 * FM_C);
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
      bh[ks] = *reinterpret_cast<const bf16x8 *>(src + 16 * ks + 8 * half);
      bl[ks] = *reinterpret_cast<const bf16x8 *>(src + FM_C + 16 * ks + 8 * half);
    }
  }

  // ---- staging: wave w fills rows 4 w .. 4 w + 3 of a tile, one 1-KiB LDS-DMA piece per row; lane = chunk POSITION in the row,
  // the chunk it fetches is position ^ (row & 15) (a permutation inside the row: the global read stays one 1-KiB line)
  const u16 *sbase = p.str + (size_t)b * p.Mps * (2 * FM_C);
  auto stage = [&](int t, int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = wave * 4 + i;
      const char *g = reinterpret_cast<const char *>(sbase + (size_t)(t * FM_TILE + row) * (2 * FM_C)) + ((lane ^ (row & 15)) << 4);
      S6D_LDS(char) *dst = (S6D_LDS(char) *)fm_smem + buf * FM_TILEB + row * FM_ROWB;
      lds_dma16(g, dst);
    }
    if (tid < FM_TILE) {
      float sv[5];
      fm_side_row<MODE>(p, b, t * FM_TILE + tid, sv);
      float *sd = reinterpret_cast<float *>(fm_smem + 2 * FM_TILEB + (t & (FM_NSIDE - 1)) * FM_SIDEB) + tid * FM_SIDE;
      *reinterpret_cast<float4 *>(sd) = make_float4(sv[0], sv[1], sv[2], sv[3]);
      sd[4] = sv[4];
    }
  };

  // ---- A fragment of stream row `col` for k-step ks: chunk 2 ks + half (hi), 32 + 2 ks + half (lo), at its permuted position
  const unsigned arow = (unsigned)(col * FM_ROWB);
  const unsigned asw = (unsigned)(col & 15);
  auto afrag = [&](int buf, int chunk) __attribute__((always_inline)) -> bf16x8 {
    return *reinterpret_cast<const bf16x8 *>(fm_smem + buf * FM_TILEB + arow + (((unsigned)chunk ^ asw) << 4));
  };
  auto tile_mfma = [&](int buf, f32x16 &acc) __attribute__((always_inline)) {
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    // fragment reads run at most 4 k-steps (8 fragments, 32 VGPRs) ahead of their MFMAs: without the fences the scheduler hoists
    // all 32 reads of the tile and spills
#pragma unroll
    for (int kg = 0; kg < 4; ++kg) {
      bf16x8 ah[4], al[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        ah[k] = afrag(buf, 2 * (4 * kg + k) + half);
        al[k] = afrag(buf, 32 + 2 * (4 * kg + k) + half);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int ks = 4 * kg + k;
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[k], bh[ks], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[k], bh[ks], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[k], bl[ks], acc, 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  // ---- per-owner running values (this lane's half of the stream rows)
  float sum = 0.f;                                                   // A: r   B: c   C: sum e^2 w2 / c
  float best = -1.f;                                                 // B, C: running arg-max key, first index wins
  int bidx = 0;
  float px = 0.f, py = 0.f, pz = 0.f;                                // C
  auto epilogue = [&](int t, const f32x16 &acc) __attribute__((always_inline)) {
    const float *side = reinterpret_cast<const float *>(fm_smem + 2 * FM_TILEB + (t & (FM_NSIDE - 1)) * FM_SIDEB);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int sr = (e & 3) + 8 * (e >> 2) + 4 * half;              // stream row of register e inside the tile
      const float *sv = side + sr * FM_SIDE;
      const float ex = __builtin_amdgcn_exp2f(acc[e]);
      if (MODE == 0) {
        sum = fmaf(ex, sv[0], sum);
      } else if (MODE == 1) {
        const float ev = ex * sv[0];
        sum += ev;
        const float key = (ev * ev) * sv[1];                         // e^2 / r_i; 0 on padding rows
        if (key > best) { best = key; bidx = t * FM_TILE + sr; }
      } else {
        const float e2 = ex * ex;
        const float key = e2 * sv[0];                                // e^2 / c_j; 0 on padding rows
        if (key > best) { best = key; bidx = t * FM_TILE + sr; }
        const float gw = e2 * sv[1];
        sum += gw;
        px = fmaf(gw, sv[2], px);
        py = fmaf(gw, sv[3], py);
        pz = fmaf(gw, sv[4], pz);
      }
      if ((e & 3) == 3) __builtin_amdgcn_sched_barrier(0);           // bounds the side-table reads in flight (register pressure)
    }
  };

  // ---- main loop ------------------------------------------------------------------------------------------------------------------
  // iteration t: stage tile t + 1; waves 0-3: matrix work of tile t, then its epilogue; waves 4-7: epilogue of tile t - 1, then the
  // matrix work of tile t.  One accumulator set per wave; the MFMA / VALU overlap comes from the two waves of a SIMD being
  // half an iteration apart.
  stage(0, 0);
  S6D_VMCNT(0);
  __syncthreads();
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  for (int t = 0; t < ntile; ++t) {
    if (t + 1 < ntile) stage(t + 1, (t + 1) & 1);
    if (wave < 4) {
      tile_mfma(t & 1, acc);
      epilogue(t, acc);
    } else {
      if (t > 0) epilogue(t - 1, acc);
      tile_mfma(t & 1, acc);
    }
    S6D_VMCNT(0);
    __syncthreads();
  }
  if (wave >= 4) epilogue(ntile - 1, acc);

  // ---- fold the two lane halves (same owner row, interleaved stream rows) and write ------------------------------------------------
  sum += __shfl_xor(sum, 32);
  if (MODE >= 1) {
    const float ob = __shfl_xor(best, 32);
    const int oi = __shfl_xor(bidx, 32);
    if (ob > best || (ob == best && oi < bidx)) { best = ob; bidx = oi; }
  }
  if (MODE == 2) {
    px += __shfl_xor(px, 32);
    py += __shfl_xor(py, 32);
    pz += __shfl_xor(pz, 32);
  }
  if (half == 0 && ovalid) {
    if (MODE == 0) {
      p.r[(size_t)b * p.ldr + orow] = sum;
    } else if (MODE == 1) {
      p.c[(size_t)b * p.ldc + orow] = sum;
      p.w2[(size_t)b * p.ldc + orow] = bidx > 0 ? 1.f : 0.f;         // label2 > 0 (model_utils.py:265,267)
    } else {
      const size_t o = (size_t)b * (p.Mo - 1) + (orow - 1);
      const float lab = bidx > 0 ? 1.f : 0.f;                        // label1 > 0 (model_utils.py:264,267)
      const float ir = 1.0f / p.r[(size_t)b * p.ldr + orow];
      const float ws = lab * (sum * ir);
      const float inv = lab * ir / (ws + 1e-6f);                     // model_utils.py:268
      p.w1[o] = lab;
      p.wsum[o] = ws;
      p.pred[o * 3] = px * inv;
      p.pred[o * 3 + 1] = py * inv;
      p.pred[o * 3 + 2] = pz * inv;
    }
  }
}

}  // namespace s6d

using namespace s6d;

static inline long fm_pad(int M) { return ((long)M + FM_TILE - 1) / FM_TILE * FM_TILE; }

extern "C" long s6d_fine_match_workspace_bytes(int B, int M1, int M2) {
  const long Mp1 = fm_pad(M1), Mp2 = fm_pad(M2);
  // xs1 | xs2 (bf16 split rows)  +  r (B, Mp1) | c (B, Mp2) | w2 (B, Mp2) | background exponentials (B, 2, max(Mp1, Mp2))   (floats)
  return (long)B * (Mp1 + Mp2) * (2 * FM_C) * 2 + ((long)B * (Mp1 + 2 * Mp2) + (long)B * 2 * (Mp1 > Mp2 ? Mp1 : Mp2)) * 4 + 256;
}

extern "C" int s6d_fine_match_f32(const float *f1, const float *f2, const float *pts2, int B, int M1, int M2, int C,
                                  float inv_temp, void *workspace, float *pred, float *wsum, float *w1, void *stream) {
  if (B < 0 || M1 < 2 || M2 < 2 || !(inv_temp > 0.f)) return S6D_EINVAL;
  if (C != FM_C || !(inv_temp <= (float)S6D_FINE_MATCH_MAX_INV_TEMP)) return S6D_EUNSUPPORTED;
  if (3.0f * inv_temp + logf((float)(M1 > M2 ? M1 : M2)) > 87.0f) return S6D_EUNSUPPORTED;      // the keys e^-3T / M must stay normal floats
  if (B == 0) return S6D_OK;
  if (!f1 || !f2 || !pts2 || !workspace || !pred || !wsum || !w1) return S6D_EINVAL;
  if (((uintptr_t)f1 | (uintptr_t)f2 | (uintptr_t)workspace) & 15) return S6D_EINVAL;
  const int Mp1 = (int)fm_pad(M1), Mp2 = (int)fm_pad(M2);
  u16 *xs1 = reinterpret_cast<u16 *>(workspace);
  u16 *xs2 = xs1 + (size_t)B * Mp1 * (2 * FM_C);
  float *r = reinterpret_cast<float *>(xs2 + (size_t)B * Mp2 * (2 * FM_C));
  float *c = r + (size_t)B * Mp1;
  float *w2 = c + (size_t)B * Mp2;
  float *ev = w2 + (size_t)B * Mp2;
  const int ldev = Mp1 > Mp2 ? Mp1 : Mp2;
  hipStream_t st = as_stream(stream);
  const float kLog2e = 1.4426950408889634f;
  hipLaunchKernelGGL(fine_split_kernel, dim3((Mp1 + 3) / 4, B), dim3(256), 0, st, f1, M1, Mp1, inv_temp * kLog2e, xs1);
  hipLaunchKernelGGL(fine_split_kernel, dim3((Mp2 + 3) / 4, B), dim3(256), 0, st, f2, M2, Mp2, 1.0f, xs2);
  hipLaunchKernelGGL(fine_bg_exp_kernel, dim3(FM_BGSPLIT, 2, B), dim3(512), 0, st, xs1, xs2, M1, M2, Mp1, Mp2, ev, ldev);
  hipLaunchKernelGGL(fine_bg_sum_kernel, dim3(2, B), dim3(64), 0, st, ev, ldev, Mp1, Mp2, r, c);
  int rc = launch_status();
  if (rc) return rc;
  FineParams p;
  p.B = B;
  p.r = r;
  p.c = c;
  p.w2 = w2;
  p.pts2 = pts2;
  p.pred = pred;
  p.wsum = wsum;
  p.w1 = w1;
  p.ldr = Mp1;
  p.ldc = Mp2;
#define FM_LAUNCH(MODE)                                                                                                 \
  do {                                                                                                                  \
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&fine_sweep_kernel<MODE>),                                 \
                              hipFuncAttributeMaxDynamicSharedMemorySize, FM_LDSB);                                     \
    hipLaunchKernelGGL((fine_sweep_kernel<MODE>), dim3(p.nblk * B), dim3(512), FM_LDSB, st, p);                         \
  } while (0)
  // sweep A: owners = rows of f1, stream = f2
  p.own = xs1; p.str = xs2; p.Mo = M1; p.Ms = M2; p.Mpo = Mp1; p.Mps = Mp2; p.nblk = (M1 - 1 + FM_OWN - 1) / FM_OWN;
  FM_LAUNCH(0);
  // sweep B: owners = rows of f2 (columns of the similarity), stream = f1
  p.own = xs2; p.str = xs1; p.Mo = M2; p.Ms = M1; p.Mpo = Mp2; p.Mps = Mp1; p.nblk = (M2 - 1 + FM_OWN - 1) / FM_OWN;
  FM_LAUNCH(1);
  // sweep C: owners = rows of f1 again
  p.own = xs1; p.str = xs2; p.Mo = M1; p.Ms = M2; p.Mpo = Mp1; p.Mps = Mp2; p.nblk = (M1 - 1 + FM_OWN - 1) / FM_OWN;
  FM_LAUNCH(2);
#undef FM_LAUNCH
  return launch_status();
}
