// Fused ViT attention with decomposed relative-position bias for the SAM image encoder (gfx950): what the kernel families share.
// A family is one header -- s6d_attn_seq.h (all-resident windows, sequences), s6d_attn_win16.h (row-padded windows of up to 16 rows),
// s6d_attn_global.h (global attention); csrc/s6d_attn.hip (bf16: all three) and csrc/s6d_attn_f16.hip (half: sequences) include them.
//
// Reference: segment_anything/modeling/image_encoder.py
//   Block.forward :166-182 (norm1 -> window_partition(pad 64->70) -> attn -> unpartition),
//   Attention.forward :224-240, add_decomposed_rel_pos :325-361, get_rel_pos :292-322.
// The reference materialises (B*25*16,196,196) / (B*16,4096,4096) fp32 score tensors plus two
// partition copies per block.  Here one kernel reads the qkv GEMM output of the 4096 REAL tokens,
// forms windows by address arithmetic (out-of-image window slots take the qkv bias as q/k/v:
// quirk Q2, padded tokens are zeros after norm1 and DO act as keys), runs flash-style online
// softmax on MFMA tiles and writes the attended tokens straight into the (B,H,W,C) map.
//
// MFMA mapping (v_mfma_f32_16x16x32_bf16, wave64):
//   S^T tile (16 keys x 16 queries) = K_tile (A: lane -> key l&15, 8 contiguous d) x Q^T (B: lane ->
//   query l&15, 8 contiguous d): the C layout then gives each lane 4 keys x 1 QUERY (col = l&15), so
//   softmax statistics are per-lane scalars (+2 shuffles across the 4 lane groups).
//   O^T tile (16 d x 16 queries)   = V^T (A, from a transposed LDS image) x P^T (B): P^T fragments
//   are exactly the exponentiated S^T registers (k-index permuted consistently on both operands),
//   so P never leaves registers and O^T keeps the per-lane query -> rescaling needs no shuffles.
//   The decomposed bias  rel_h[q,ky] + rel_w[q,kx]  comes from two per-query tables
//   T[j][q] = rel_pos[j] . q  (2S-1 entries) built with the same MFMA shape in the strip prologue.
#pragma once
#include "s6d_bf16.h"

// Element type of q / k / v / P / the output.  The headers are compiled for two element types: from csrc/s6d_attn.hip for bf16 (SAM,
// DINOv2: `bf16x8`, `f2bf` mean what they say), and from csrc/s6d_attn_f16.hip with S6D_ATTN_F16 = 1 for IEEE half (the PEM's ViT-B,
// round 3): the same code in namespace s6d_h with v_mfma_f32_16x16x32_f16, where the names below stand for the half forms and only
// the sequence family (s6d_seq_attention_f16, s6d_seq_attention_strided_f16) is built.  Nothing else depends on the element's bit
// layout (probabilities are <= 1, sums are fp32).
#ifndef S6D_ATTN_F16
#define S6D_ATTN_F16 0
#endif
#if S6D_ATTN_F16
#define S6D_ATTN_NS s6d_h
#define S6D_ATTN_MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0)
#define S6D_ATTN_ONE 0x3C00
#else
#define S6D_ATTN_NS s6d
#define S6D_ATTN_MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0)
#define S6D_ATTN_ONE 0x3F80
#endif

namespace S6D_ATTN_NS {
using namespace s6d;

// bf16: bf16x8 is csrc/s6d_bf16.h's and the conversions forward to its pair; half: this namespace's own forms under the same names
#if S6D_ATTN_F16
typedef f16x8 bf16x8;
__device__ __forceinline__ u16 f2bf(float f) {  // round-to-nearest-even
  union { _Float16 b; u16 u; } x;
  x.b = (_Float16)f;
  return x.u;
}
__device__ __forceinline__ float bf2f(u16 h) {
  union { _Float16 b; u16 u; } x;
  x.u = h;
  return (float)x.b;
}
#else
__device__ __forceinline__ u16 f2bf(float f) { return bf16_bits(f); }
__device__ __forceinline__ float bf2f(u16 h) { return bf16_value(h); }
#endif

struct AttnParams {
  const u16 *qkv;      // (B,H,W,3,nh,HD) bf16
  const u16 *qkv_bias; // (3,nh,HD) bf16  (q/k/v of out-of-image window slots)
  const u16 *rel_h;    // (2S-1,HD) bf16 or nullptr
  const u16 *rel_w;    // (2S-1,HD) bf16
  u16 *out;            // (B,H,W,nh,HD) bf16
  int B, H, W, nh;
  int ws;              // window size (0 = global attention over the H x W grid)
  int S;               // side of the attention grid (ws, or H for global)
  int T;               // tokens per attention problem = S*S
  int nwx, nwy;        // windows per image along x / y (1,1 for global)
  int LT;              // padded table length (multiple of 16, >= 2S-1)
  unsigned magicS;     // ceil(2^32 / S): n / S == umulhi(n, magicS) for n < 2^32 / S
  float scale_log2;    // softmax scale * log2(e): scores live in the exp2 domain
  // q/k/v element (token, which, head, d) sits at qkv + token * tok_stride + which * which_stride + head * head_stride + d.
  //   token-major (the raw Linear output (B,H,W,3,nh,HD)): tok_stride = 3 nh HD, which_stride = nh HD, head_stride = HD
  //   head-major  ((3, nh, B H W, HD), written by the qkv GEMM's column-block epilogue): tok_stride = HD, head_stride = B H W HD,
  //               which_stride = nh B H W HD -- a head's rows of one window row / key tile are contiguous whole lines
  long tok_stride, which_stride, head_stride;
};

__device__ __forceinline__ const u16 *qkv_at(const AttnParams &p, size_t tok, int which, int head) {
  return p.qkv + tok * (size_t)p.tok_stride + (size_t)which * (size_t)p.which_stride + (size_t)head * (size_t)p.head_stride;
}

// Ablation switches for profiling are COMPILE-time (-DS6D_ATTN_ABLATE=mask through S6D_EXTRA_HIPCC_FLAGS): 1 = no K/V
// loads, 2 = no tile math, 4 = no softmax arithmetic, 8 = no PV, 16 = no QK^T, 32 = no LDS stores of the staged tile.  As run-time branches they cut the
// tile loop into a dozen basic blocks and kept the scheduler from placing MFMAs beside the softmax VALU work.
#ifndef S6D_ATTN_ABLATE
#define S6D_ATTN_ABLATE 0
#endif
constexpr int kAbl = S6D_ATTN_ABLATE;
// The global kernels and the persistent window kernel store their K images (13 chunks per row) chunk-swizzled -- kswz() of
// csrc/s6d_bf16.h, KSWZ = true below; the all-resident window kernels do not.
// S6D_G64_TIMING (probe build of the global64 and the persistent window kernel; process_tile carries two of its clock reads; writes 320 bytes BEHIND the output tensor, which tools/attn_time.py allocates): shader-clock totals per phase of attn_global64_kernel's tile loop,
// per wave of workgroup 0: [barrier wait | DMA issue | QK^T + scale + max | exp + pack | P V]  (tools/attn_time.py prints them)
#ifndef S6D_G64_TIMING
#define S6D_G64_TIMING 0
#endif
#if S6D_G64_TIMING
#define S6D_TICK(tk, i)                                  \
  do {                                                   \
    __builtin_amdgcn_sched_barrier(0);                   \
    (tk)[i] = (long long)__builtin_amdgcn_s_memtime();   \
    __builtin_amdgcn_sched_barrier(0);                   \
  } while (0)
#else
#define S6D_TICK(tk, i) do { } while (0)
#endif

constexpr float kLog2e = 1.4426950408889634f;
// v_exp_f32 without the denormal-range fix-up of fast_exp2(): arguments here are <= 2^kDefer and tiny results may flush
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

template <int HD>
struct Cfg {
  static constexpr int KS = (HD + 31) / 32;     // k-steps of 32 over the head dim (zero padded)
  static constexpr int HDP = KS * 32;           // padded head dim
  static constexpr int DT = HD / 16;            // 16-wide d tiles of the output
  static constexpr int KROW = HDP + 8;          // K image row stride (bf16 elements): +16 B pad
  // V image row stride (row-major [key][d]): an ODD multiple of 16 elements (32 B), so the 8 key rows that one
  // half-wave of a ds_read_b64_tr_b16 touches start on 8 distinct 32-byte bank groups (HD + 8 was 2-way conflicted)
  // Head dim 64 takes HD + 8 instead (144-byte rows: the eighth row of a half-wave wraps onto the first one's first four banks, a
  // 2-way conflict on one row in eight) -- at 160 bytes the K / V images of a 257-token sequence miss the 80 KiB that lets TWO
  // workgroups share a CU by 3 KiB (round 4, attn_window_kernel's compact layout).
  static constexpr int VROW = HD == 64 ? HD + 8 : (((HD + 15) / 16) | 1) * 16;
  static constexpr int KT = 64;                 // keys per tile
  static constexpr int KPARTS = HDP / 8, VPARTS = HD / 8;
};

__device__ __forceinline__ int div_S(const AttnParams &p, int n) { return (int)__umulhi((unsigned)n, p.magicS); }

// global token index of slot `t` of problem (b, wy, wx); false for an out-of-image / out-of-range slot
// (`off` is always a valid token index -- clamped -- so loads through it may be issued unconditionally)
__device__ __forceinline__ bool token_offset(const AttnParams &p, int b, int wy, int wx, int t, size_t &off) {
  if (p.ws == 0) {                      // global attention: slots are the image tokens in raster order
    off = (size_t)b * p.T + min(t, p.T - 1);
    return t < p.T;
  }
  const int ty = div_S(p, t), tx = t - ty * p.S;
  const int y = wy * p.ws + ty, x = wx * p.ws + tx;
  const bool in = (y < p.H) && (x < p.W) && (t < p.T);
  // sequences (no qkv_bias: s6d_seq_attention_*) stage a slot past the end from their OWN first token, which load_chunk then reads:
  // the padded query rows of the last strip take part in process_tile's wave-wide rescale vote, so their values reach the real rows'
  // rounding; taken from another sequence of the launch, they made a sequence's result depend on its neighbours
  off = (in || p.qkv_bias) ? ((size_t)(b * p.H + min(y, p.H - 1)) * p.W + min(x, p.W - 1)) : (size_t)b * p.H * p.W;
  return in;
}

// 8 consecutive head-dim elements [d0, d0+8) of q/k/v (which = 0/1/2) for a token slot.  Branch-free on
// purpose: the load is unconditional (clamped address, pointer select), zeros are selected afterwards, so the
// compiler can keep a whole batch of these in flight instead of one exec-masked load + vmcnt(0) each.
// `tok` must be a valid token index even when !valid (callers clamp).
template <int HD>
__device__ __forceinline__ uint4 load_chunk(const AttnParams &p, int which, int head, bool valid, size_t tok, int d0) {
  const int C = p.nh * HD;
  const int dc = d0 < HD ? d0 : HD - 8;
  const u16 *a = qkv_at(p, tok, which, head) + dc;
  const u16 *bsrc = p.qkv_bias ? p.qkv_bias + (size_t)which * C + head * HD + dc : a;       // (sequences: see token_offset)
  const uint4 v = *reinterpret_cast<const uint4 *>(valid ? a : bsrc);
  return d0 < HD ? v : make_uint4(0, 0, 0, 0);
}

// MODE 0: bias from per-query LDS tables th/tw (any S);  MODE 1: aligned fast path (S == 64, one key row per
// tile): th value is one LDS word per tile, tw lives in 16 registers;  MODE 2: no positional bias.
//   Kl : K image of the tile [64][KROW];  Vl : V image of the tile [64][VROW] (row-major, read with
//   ds_read_b64_tr_b16: lane c of a 16-lane group receives column c of a 4-key block).
// NS query strips (16 queries each) are processed against the same K / V fragments: every LDS operand read
// feeds NS MFMAs.
template <int HD, int NS>
struct StripState {
  bf16x8 qf[NS][Cfg<HD>::KS];
  float twr[NS][16];
  float m_run[NS];
  f32x4 lacc[NS];                          // running row sums: every element of lacc[n] is the sum for query lane & 15
  f32x4 oacc[NS][Cfg<HD>::DT];
  const float *th[NS], *tw[NS];
  int qy[NS], qx[NS];
};

// SUBS: 16-key sub-tiles of this tile that exist (a sequence's tail tile: 257 keys = 4 tiles + 1 sub-tile): the score MFMAs of the
// others are skipped (their probabilities are 0) and the PV pass covers ceil(SUBS / 2) 32-key steps; the V image must hold finite
// values for the absent keys of the last step.
template <int HD, int MODE, int NS, bool KSWZ = false, bool PRIO = false, int SUBS = 4>
__device__ __forceinline__ void process_tile(const AttnParams &p, const u16 *Kl, const u16 *Vl, int key0,
                                             StripState<HD, NS> &st, const float (&thv)[NS], int lane, long long *tk = nullptr) {
  using C = Cfg<HD>;
  static_assert(SUBS >= 1 && SUBS <= 4, "a tile has four 16-key sub-tiles");
  const int g = lane >> 4, c = lane & 15;
  const int gk = KSWZ ? (g ^ kswz(c)) : g;               // chunk of this lane's K fragment inside its group of 4 (see kswz())
  float s[NS][4][4];
  if (PRIO) __builtin_amdgcn_s_setprio(1);
  auto kfrag = [&](int sub, int ks) __attribute__((always_inline)) {
    return *reinterpret_cast<const bf16x8 *>(Kl + (sub * 16 + c) * C::KROW + ks * 32 + gk * 8);
  };
#pragma unroll
  for (int sub = 0; sub < 4; ++sub) {
    f32x4 acc[NS];
#pragma unroll
    for (int n = 0; n < NS; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (sub >= SUBS) {
#pragma unroll
      for (int n = 0; n < NS; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) s[n][sub][r] = -1e30f;
      continue;
    }
    if (!(kAbl & 16)) {
#pragma unroll
      for (int ks = 0; ks < C::KS; ++ks) {
        const bf16x8 a = kfrag(sub, ks);
#pragma unroll
        for (int n = 0; n < NS; ++n) acc[n] = S6D_ATTN_MFMA16(a, st.qf[n][ks], acc[n]);
      }
    }
#pragma unroll
    for (int n = 0; n < NS; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = acc[n][r] * p.scale_log2;
        if (MODE == 1) {
          s[n][sub][r] = v + st.twr[n][sub * 4 + r];      // thv (constant over the tile for this lane) joins the max only
        } else {
          const int kk = key0 + sub * 16 + g * 4 + r;     // key slot of this score; query = lane & 15
          if (MODE == 0) {
            const int ky = div_S(p, kk), kx = kk - ky * p.S;
            const int jh = min(max(st.qy[n] - ky + p.S - 1, 0), p.LT - 1), jw = st.qx[n] - kx + p.S - 1;
            v += st.th[n][c * p.LT + jh] + st.tw[n][c * p.LT + jw];
          }
          s[n][sub][r] = kk < p.T ? v : -1e30f;
        }
      }
  }
  union PB { bf16x8 v; u16 h[8]; };
  PB pb[NS][2];
  union VA { bf16x8 v; s16x4 q[2]; };
  if (PRIO) __builtin_amdgcn_s_setprio(0);
  if (kAbl & 4) {                                          // ablation: no softmax arithmetic
#pragma unroll
    for (int n = 0; n < NS; ++n)
#pragma unroll
      for (int sub = 0; sub < 4; ++sub)
#pragma unroll
        for (int r = 0; r < 4; ++r) pb[n][sub >> 1].h[(sub & 1) * 4 + r] = f2bf(s[n][sub][r]);
  } else {
    // deferred rescaling: keep the old running max while no query's max grew by more than 2^kDefer (P stays
    // <= 2^kDefer, exact in bf16's exponent range); the O / l rescale is skipped on those tiles.  Both strips'
    // decisions are taken first, so the (rare) rescale is ONE wave-uniform branch and the rest of the tile is
    // straight-line code the scheduler can interleave with the MFMAs.
    constexpr float kDefer = 6.0f;
    float mx[NS];
    bool grow[NS], any_grow = false;
#pragma unroll
    for (int n = 0; n < NS; ++n) {
      float v = s[n][0][0];
#pragma unroll
      for (int sub = 0; sub < SUBS; ++sub)
#pragma unroll
        for (int r = 0; r < 4; ++r) v = fmaxf(v, s[n][sub][r]);
      v = fmaxf(v, __shfl_xor(v, 16));
      v = fmaxf(v, __shfl_xor(v, 32));
      if (MODE == 1) v += thv[n];                             // true score maximum of the tile
      mx[n] = v;
      grow[n] = __any(v - st.m_run[n] > kDefer);
      any_grow |= grow[n];
    }
    S6D_TICK(tk, 3);
    if (any_grow) {                                           // wave-uniform
#pragma unroll
      for (int n = 0; n < NS; ++n)
        if (grow[n]) {
          const float m_new = fmaxf(st.m_run[n], mx[n]);
          const float alpha = fast_exp2(st.m_run[n] - m_new);
          st.lacc[n] *= alpha;
#pragma unroll
          for (int dt = 0; dt < C::DT; ++dt) st.oacc[n][dt] *= alpha;
          st.m_run[n] = m_new;
        }
    }
#pragma unroll
    for (int n = 0; n < NS; ++n) {
      const float m_sub = (MODE == 1) ? st.m_run[n] - thv[n] : st.m_run[n];
#pragma unroll
      for (int sub = 0; sub < 4; ++sub)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          pb[n][sub >> 1].h[(sub & 1) * 4 + r] = sub < SUBS ? f2bf(fast_exp2(s[n][sub][r] - m_sub)) : (u16)0;
    }
  }
  // O^T += V^T P^T: k-step j covers keys [32j, 32j+32); MFMA k-index e<4 -> key 32j+g*4+e, e>=4 -> 32j+16+g*4+(e-4).
  // The row sums ride the matrix core too: an all-ones A fragment makes every row of lacc the sum over keys of the
  // SAME bf16-rounded P that multiplies V (no VALU adds, no lane exchange).
  if (kAbl & 8) {                                          // ablation: no PV (keep P live)
#pragma unroll
    for (int n = 0; n < NS; ++n) st.lacc[n][0] += (float)pb[n][0].h[0] + (float)pb[n][1].h[7];
    return;
  }
  union { bf16x8 v; u16 h[8]; } ones;
#pragma unroll
  for (int i = 0; i < 8; ++i) ones.h[i] = S6D_ATTN_ONE;            // 1.0 in the element type
  S6D_TICK(tk, 4);
  if (PRIO) __builtin_amdgcn_s_setprio(1);
#pragma unroll
  for (int j = 0; j < (SUBS + 1) / 2; ++j) {
    const u16 *vrow = Vl + (32 * j + g * 4 + (c >> 2)) * C::VROW + (c & 3) * 4;
#pragma unroll
    for (int n = 0; n < NS; ++n) st.lacc[n] = S6D_ATTN_MFMA16(ones.v, pb[n][j].v, st.lacc[n]);
#pragma unroll
    for (int dt = 0; dt < C::DT; ++dt) {
      VA va;
      va.q[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((S6D_LDS(s16x4) *)(vrow + dt * 16));
      va.q[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((S6D_LDS(s16x4) *)(vrow + 16 * C::VROW + dt * 16));
#pragma unroll
      for (int n = 0; n < NS; ++n)
        st.oacc[n][dt] = S6D_ATTN_MFMA16(va.v, pb[n][j].v, st.oacc[n][dt]);
    }
  }
  if (PRIO) __builtin_amdgcn_s_setprio(0);
}

// Range guard of the passes that keep a FIXED reference instead of a running maximum (process_tile_nomax, win16_pass_stream): a row
// is redone (second pass / raised reference) when its sum of P = exp2(s - m) is not below 2^100 (inf / NaN included) OR when one of
// its O^T accumulators is not finite (the accumulators hold sum P V, i.e. up to 2^100 |V|, and overflowed float32 for
// |V| above 2^28 while the sum still passed; tests/test_gpu_attn.py runs |V| = 2^50 under P up to 2^90).  A lower sum limit instead
// (2^60 was tried) sends ordinary frames through the second pass: the seeded ViT-H of the benched step has rows 60 .. 100 log2
// units above their first tile, and the global kernel went 1.81 -> 3.25 ms.
constexpr float kNoMaxSumLimit = 1.2676506e30f;                    // 2^100
constexpr float kNoMaxFinite = 3.0e38f;

// ---- round 5: the 64 x 64 global tile WITHOUT a running maximum ---------------------------------------------------------------
// process_tile spends, per score, scale + bias (fma), running max (max / max3), subtract, exp2 and half a pack, plus two
// cross-lane exchanges and a wave vote per strip for the maximum -- 130 VALU + 32 exp2 beside 48 matrix instructions per tile, and
// the maximum is a barrier between ALL score instructions of a tile and ALL its exponentials.  None of the maximum is needed
// after the first tile: P only has to stay representable.  bf16 has float32's exponent range and the accumulators (row sums on
// the matrix core, O^T) are float32, so with m fixed at the FIRST tile's row maximum P = exp2(s - m) is computed to the same
// relative precision as with a running maximum as long as no row's sum approaches 2^127.  So after tile 0 (process_tile, which
// sets m_run):
//   * the rel-pos column bias rides the matrix core: the score chain starts from C = tw / scale_log2 instead of 0;
//   * P = exp2(fma(acc, scale_log2, th - m)): ONE fma per score; no max, no subtract, no exchange, no vote, no rescale branch, and
//     the exponentials of sub-tile s are independent of the score instructions of sub-tile s + 1;
//   * at the end of the tile loop a row sum that is not < kNoMaxSumLimit = 2^100 (inf / NaN included), or a non-finite accumulator, makes the WORKGROUP run its tile loop again
//     with process_tile for every tile (attn_global64_kernel): the old arithmetic is the fallback, so any input the old kernel
//     handled is still handled -- scores that grow by more than 2^100 over the first 64 keys' maximum take the slow path.
// (s_setprio 1 around this tile's matrix instructions, as process_tile's PRIO does, measured 0 on it: docs/NOTEBOOK_r5.md,
// profiles/r05_attn_nomax_variants.txt.)
template <int HD, int NS, bool KSWZ>
__device__ __forceinline__ void process_tile_nomax(const AttnParams &p, const u16 *Kl, const u16 *Vl, StripState<HD, NS> &st,
                                                   const f32x4 (&cbias)[NS][4], const float (&nb)[NS], int lane) {
  using C = Cfg<HD>;
  const int g = lane >> 4, c = lane & 15;
  const int gk = KSWZ ? (g ^ kswz(c)) : g;
  union PB { bf16x8 v; u16 h[8]; };
  PB pb[NS][2];
#pragma unroll
  for (int sub = 0; sub < 4; ++sub) {
    f32x4 acc[NS];
#pragma unroll
    for (int n = 0; n < NS; ++n) acc[n] = cbias[n][sub];
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks) {
      const bf16x8 a = *reinterpret_cast<const bf16x8 *>(Kl + (sub * 16 + c) * C::KROW + ks * 32 + gk * 8);
#pragma unroll
      for (int n = 0; n < NS; ++n) acc[n] = S6D_ATTN_MFMA16(a, st.qf[n][ks], acc[n]);
    }
#pragma unroll
    for (int n = 0; n < NS; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r)     // (scalar FMAs on purpose: as two v_pk_fma_f32 per lane the kernel measured 1.6 % slower, profiles/r05_attn_pkfma_ab.txt)
        pb[n][sub >> 1].h[(sub & 1) * 4 + r] = f2bf(fast_exp2(__builtin_fmaf(acc[n][r], p.scale_log2, nb[n])));
  }
  union { bf16x8 v; u16 h[8]; } ones;
#pragma unroll
  for (int i = 0; i < 8; ++i) ones.h[i] = S6D_ATTN_ONE;
  union VA { bf16x8 v; s16x4 q[2]; };
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const u16 *vrow = Vl + (32 * j + g * 4 + (c >> 2)) * C::VROW + (c & 3) * 4;
#pragma unroll
    for (int n = 0; n < NS; ++n) st.lacc[n] = S6D_ATTN_MFMA16(ones.v, pb[n][j].v, st.lacc[n]);
#pragma unroll
    for (int dt = 0; dt < C::DT; ++dt) {
      VA va;
      va.q[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((S6D_LDS(s16x4) *)(vrow + dt * 16));
      va.q[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((S6D_LDS(s16x4) *)(vrow + 16 * C::VROW + dt * 16));
#pragma unroll
      for (int n = 0; n < NS; ++n) st.oacc[n][dt] = S6D_ATTN_MFMA16(va.v, pb[n][j].v, st.oacc[n][dt]);
    }
  }
}

// ---- staging: global -> registers -> LDS, split so the loads can fly under the previous tile's math ------
template <int HD, int THREADS>
struct Stager {
  using C = Cfg<HD>;
  static constexpr int NK = (64 * C::KPARTS + THREADS - 1) / THREADS;
  static constexpr int NV = (64 * C::VPARTS + THREADS - 1) / THREADS;
  uint4 k[NK], v[NV];

  __device__ __forceinline__ void load(const AttnParams &p, int b, int wy, int wx, int head, int key0, int tid) {
#pragma unroll
    for (int n = 0; n < NK; ++n) {
      const int i = min(tid + n * THREADS, 64 * C::KPARTS - 1);     // surplus lanes repeat the last chunk
      const int key = i / C::KPARTS, part = i - key * C::KPARTS;
      size_t tok;
      const bool valid = token_offset(p, b, wy, wx, key0 + key, tok);
      k[n] = load_chunk<HD>(p, 1, head, valid, tok, part * 8);
    }
#pragma unroll
    for (int n = 0; n < NV; ++n) {
      const int i = min(tid + n * THREADS, 64 * C::VPARTS - 1);
      const int key = i / C::VPARTS, part = i - key * C::VPARTS;
      size_t tok;
      const bool valid = token_offset(p, b, wy, wx, key0 + key, tok);
      v[n] = load_chunk<HD>(p, 2, head, valid, tok, part * 8);
    }
  }
  // klim / vlim: rows of this tile that the image holds (a compact image ends inside the last tile)
  __device__ __forceinline__ void store(u16 *Kl, u16 *Vl, int tid, int klim = 64, int vlim = 64) const {
#pragma unroll
    for (int n = 0; n < NK; ++n) {
      const int i = tid + n * THREADS;
      const int key = i / C::KPARTS, part = i - key * C::KPARTS;
      if (i < 64 * C::KPARTS && key < klim) *reinterpret_cast<uint4 *>(Kl + key * C::KROW + part * 8) = k[n];
    }
#pragma unroll
    for (int n = 0; n < NV; ++n) {
      const int i = tid + n * THREADS;
      const int key = i / C::VPARTS, part = i - key * C::VPARTS;
      if (i < 64 * C::VPARTS && key < vlim) *reinterpret_cast<uint4 *>(Vl + key * C::VROW + part * 8) = v[n];
    }
  }
};

// Global attention, T % 64 == 0: token slots are contiguous in memory, so each thread's chunk addresses are
// fixed up to a per-tile stride -- pointers and LDS offsets are computed once, a tile costs 6 loads + 6 adds.
// K rows are stored chunk-swizzled (kswz).  The alternative was the unswizzled image (S6D_GLB_KSWZ = 0): 1.89 against 1.81 ms with
// the swizzle and the 65-float th stride together (docs/NOTEBOOK_r1_r4.md section 4.2, profiles/r02_attn_variants.txt).
template <int HD, int THREADS>
struct StagerLinear {
  using C = Cfg<HD>;
  static constexpr int NK = (64 * C::KPARTS + THREADS - 1) / THREADS;
  static constexpr int NV = (64 * C::VPARTS + THREADS - 1) / THREADS;
  uint4 k[NK], v[NV];
  const u16 *kp[NK], *vp[NV];
  // LDS element offsets from the ring slot's K image.  Surplus lanes (chunk counts are not multiples of the
  // workgroup size) store into the unused 16-byte pad that ends each K row, so every store is unconditional:
  // exec-masked stores would cut the tile loop into extra basic blocks.
  int ko[NK], vo[NV];
  bool kz[NK];                           // chunk lies in the zero padding of the head dim
  static_assert(Cfg<HD>::KROW - Cfg<HD>::HDP == 8, "K rows end in a 16-byte pad");

  __device__ __forceinline__ void init(const AttnParams &p, int b, int head, int tid) {
#pragma unroll
    for (int n = 0; n < NK; ++n) {
      const int i = tid + n * THREADS, ic = min(i, 64 * C::KPARTS - 1);
      const int key = ic / C::KPARTS, part = ic - key * C::KPARTS;
      kz[n] = part * 8 >= HD;
      kp[n] = qkv_at(p, (size_t)b * p.T + key, 1, head) + (kz[n] ? HD - 8 : part * 8);
      ko[n] = i < 64 * C::KPARTS ? key * C::KROW + (part ^ kswz(key)) * 8 : (tid & 63) * C::KROW + C::HDP;
    }
#pragma unroll
    for (int n = 0; n < NV; ++n) {
      const int i = tid + n * THREADS, ic = min(i, 64 * C::VPARTS - 1);
      const int key = ic / C::VPARTS, part = ic - key * C::VPARTS;
      vp[n] = qkv_at(p, (size_t)b * p.T + key, 2, head) + part * 8;
      vo[n] = i < 64 * C::VPARTS ? 64 * C::KROW + key * C::VROW + part * 8 : (tid & 63) * C::KROW + C::HDP;
    }
  }
  __device__ __forceinline__ void load(size_t tile_stride_elems, int t) {
#pragma unroll
    for (int n = 0; n < NK; ++n) k[n] = *reinterpret_cast<const uint4 *>(kp[n] + tile_stride_elems * t);
#pragma unroll
    for (int n = 0; n < NV; ++n) v[n] = *reinterpret_cast<const uint4 *>(vp[n] + tile_stride_elems * t);
  }
  __device__ __forceinline__ void store(u16 *Kl) const {            // Kl: K image of the ring slot, V image right behind
#pragma unroll
    for (int n = 0; n < NK; ++n) *reinterpret_cast<uint4 *>(Kl + ko[n]) = kz[n] ? make_uint4(0, 0, 0, 0) : k[n];
#pragma unroll
    for (int n = 0; n < NV; ++n) *reinterpret_cast<uint4 *>(Kl + vo[n]) = v[n];
  }
};

template <int HD>
__device__ __forceinline__ void load_q(const AttnParams &p, int b, int wy, int wx, int head, int q0,
                                       bf16x8 (&qf)[Cfg<HD>::KS], int lane) {
  const int g = lane >> 4, c = lane & 15;
  size_t tok;
  const bool valid = token_offset(p, b, wy, wx, q0 + c, tok);
#pragma unroll
  for (int ks = 0; ks < Cfg<HD>::KS; ++ks) {
    union { uint4 u; bf16x8 v; } x;
    x.u = load_chunk<HD>(p, 0, head, valid, tok, ks * 32 + g * 8);
    qf[ks] = x.v;
  }
}

// dst[c*ld + jj] = log2(e) * rel[j0 + sgn*jj] . q_c   for jj in [0, 16*njt).  `rel` is the zero-padded copy
// [rows >= max j + 1][HDP] made by pad_rel_kernel, so every load is unconditional: all njt*KS loads of a table
// are issued back to back (the bounds-checked form compiled to one exec-masked load + vmcnt(0) per MFMA).
template <int HD, int NJT>
__device__ __forceinline__ void build_table(const u16 *rel, int j0, int sgn, const bf16x8 (&qf)[Cfg<HD>::KS],
                                            float *dst, int ld, int lane) {
  using C = Cfg<HD>;
  const int g = lane >> 4, c = lane & 15;
  union { uint4 u; bf16x8 v; } r[NJT][C::KS];
#pragma unroll
  for (int jt = 0; jt < NJT; ++jt) {
    const int j = j0 + sgn * (jt * 16 + c);
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks)
      r[jt][ks].u = *reinterpret_cast<const uint4 *>(rel + (size_t)j * C::HDP + ks * 32 + g * 8);
  }
#pragma unroll
  for (int jt = 0; jt < NJT; ++jt) {
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks) a = S6D_ATTN_MFMA16(r[jt][ks].v, qf[ks], a);
    // C layout: row jj = jt*16 + g*4 + r, col = query c
    float *o = dst + c * ld + jt * 16 + g * 4;
    if ((ld & 3) == 0) {
      *reinterpret_cast<float4 *>(o) = make_float4(a[0] * kLog2e, a[1] * kLog2e, a[2] * kLog2e, a[3] * kLog2e);
    } else {                                              // odd strides (bank spreading): rows are not 16-byte aligned
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = a[r] * kLog2e;
    }
  }
}

template <int HD>
__device__ __forceinline__ void store_strip(const AttnParams &p, int b, int wy, int wx, int head, int q0, float l_run,
                                            const f32x4 (&oacc)[Cfg<HD>::DT], int lane) {
  const int g = lane >> 4, c = lane & 15;
  size_t tok;
  if (!token_offset(p, b, wy, wx, q0 + c, tok)) return;
  const float inv = 1.0f / l_run;
  u16 *dst = p.out + tok * (size_t)(p.nh * HD) + head * HD;
#pragma unroll
  for (int dt = 0; dt < Cfg<HD>::DT; ++dt) {
    union { uint2 u; u16 h[4]; } o;
#pragma unroll
    for (int r = 0; r < 4; ++r) o.h[r] = f2bf(oacc[dt][r] * inv);
    *reinterpret_cast<uint2 *>(dst + dt * 16 + g * 4) = o.u;   // O^T rows g*4..g*4+3 = 4 consecutive d
  }
}

// Work item id -> (image, window, head).  All heads of a window read the same token rows (each head a 160-byte run
// of every 7.7 KB row), so they should run on ONE XCD at about the same time: consecutive ids go round-robin over
// the 8 XCDs (observed placement: id % 8), and an XCD's ids walk head-fastest through ITS windows -- the other heads'
// halves of every cache line then hit that XCD's L2 instead of being fetched from HBM once per XCD.
struct WinItem {
  int b, wy, wx, head;
  __device__ __forceinline__ void decode(const AttnParams &p, int id) {
    const int nwin = p.B * p.nwy * p.nwx, cut = (nwin & ~7) * p.nh;
    int win;
    if (id < cut) {
      const int xcd = id & 7, loc = id >> 3;
      head = loc % p.nh;
      win = (loc / p.nh) * 8 + xcd;
    } else {
      head = id % p.nh;
      win = id / p.nh;
    }
    wx = win % p.nwx; win /= p.nwx;
    wy = win % p.nwy; win /= p.nwy;
    b = win;
  }
};

// ---- LDS-DMA (the persistent window kernel and the global64 kernel) --------------------------------------------------------------
// Both issue their pieces with lds_dma16_m0 and wait with S6D_VMCNT / S6D_LGKM0 (csrc/s6d_mem.h; the functions there are namespace
// s6d's in both element-type builds, found through the using-directive above).
__device__ const uint4 g_attn_zero16 = {0u, 0u, 0u, 0u};          // the 16-byte zero that padded / out-of-window chunks are DMA'd from

// launch with `lds` bytes of dynamic LDS: above 64 KiB a kernel needs the attribute first
template <class... P, class... A>
static void launch_lds(void (*kernel)(P...), unsigned grid, unsigned block, size_t lds, hipStream_t st, A... args) {
  (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds, st, args...);
}

}  // namespace S6D_ATTN_NS
