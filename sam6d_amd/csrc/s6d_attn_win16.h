// Row-padded window attention, windows of up to 16 x 16 tokens with the decomposed position bias (SAM's 14 x 14): key slot = ky * 16 + kx.
// attn_window16_kernel takes one (window, head) item per workgroup; attn_window16p_kernel is persistent, next item prefetched by LDS-DMA.
#pragma once
#include "s6d_attn_common.h"

namespace S6D_ATTN_NS {

#ifndef S6D_WIN16_STREAM
#define S6D_WIN16_STREAM 1           // 14 x 14 windows: one streaming pass without the exact maximum (win16_pass_stream), exact pass as the fallback
#endif
#ifndef S6D_WIN16_KSWZ
#define S6D_WIN16_KSWZ 1             // the chunk swizzle of kswz() on the persistent window kernel's compact K image (11-chunk rows).  Round 2 measured
                                     // it at 0.265 against 0.260 ms (the swizzled source computed per DMA instruction); since round 5 the per-lane
                                     // chunk map is made once per kernel and the swizzle is free: 0.2403 -> 0.2372 ms (profiles/r05_attn_window_stream.txt)
#endif

template <int HD>
struct RelFrags {                                                   // MFMA A fragments of the padded position tables, rows 0..31
  union { uint4 u; bf16x8 v; } rh[2][Cfg<HD>::KS], rw[2][Cfg<HD>::KS];
  __device__ __forceinline__ void load(const AttnParams &p, int lane) {
    using C = Cfg<HD>;
    const int g = lane >> 4, c = lane & 15;
#pragma unroll
    for (int jt = 0; jt < 2; ++jt)
#pragma unroll
      for (int ks = 0; ks < C::KS; ++ks) {
        rh[jt][ks].u = *reinterpret_cast<const uint4 *>(p.rel_h + (size_t)(jt * 16 + c) * C::HDP + ks * 32 + g * 8);
        rw[jt][ks].u = *reinterpret_cast<const uint4 *>(p.rel_w + (size_t)(jt * 16 + c) * C::HDP + ks * 32 + g * 8);
      }
  }
};

constexpr int W16_LT = 36;   // scratch table row stride (floats): 144 B rows keep the float4 writes and the per-query
                             // word reads (16 distinct rows per instruction) on distinct banks; 32 was 8-way conflicted

// Bias registers of NR query rows: rel_w / rel_h dot q through the wave's own LDS scratch `tab` ([16][W16_LT]
// floats, reused table after table: same-wave LDS operations execute in order).  Per lane (query c, group g):
//   twr[n][r]  = log2e * rel_w[c - kx + S - 1] . q_c, kx = g*4 + r   (-1e30 for kx >= S: the column mask)
//   thv[n][ky] = log2e * rel_h[qy_n - ky + S - 1] . q_c             (-1e30 for ky >= S: the row mask)
// Depends only on Q and the position tables: the kernel runs it while the K / V staging loads are in flight.
template <int HD, int NR, int SRC>
__device__ __forceinline__ void win16_tables(const RelFrags<HD> &rf, int S, int qy0, int rstride,
                                             const bf16x8 (*qf)[Cfg<HD>::KS], float *tab, float (*twr)[4],
                                             float (*thv)[16], int lane) {
  using C = Cfg<HD>;
  const int g = lane >> 4, c = lane & 15;
#pragma unroll
  for (int n = 0; n < NR; ++n) {
    const int qy = min(qy0 + n * rstride, S - 1);                   // an out-of-window second row is computed, not stored
    f32x4 ah[2], aw[2];
#pragma unroll
    for (int jt = 0; jt < 2; ++jt) {
      ah[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
      aw[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < C::KS; ++ks) {
        aw[jt] = S6D_ATTN_MFMA16(rf.rw[jt][ks].v, qf[n][ks], aw[jt]);
        ah[jt] = S6D_ATTN_MFMA16(rf.rh[jt][ks].v, qf[n][ks], ah[jt]);
      }
    }
    // C layout: row jj = jt*16 + g*4 + r, col = query c
#pragma unroll
    for (int jt = 0; jt < 2; ++jt)
      *reinterpret_cast<float4 *>(tab + c * W16_LT + jt * 16 + g * 4) =
          make_float4(aw[jt][0] * kLog2e, aw[jt][1] * kLog2e, aw[jt][2] * kLog2e, aw[jt][3] * kLog2e);
    S6D_WAVE_RENDEZVOUS();   // (same-wave LDS order; on the GPU the wave's LDS operations execute in program order)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int kx = g * 4 + r;
      const float v = tab[c * W16_LT + min(max(c - kx + S - 1, 0), 31)];
      twr[n][r] = (kx < S && c < S) ? v : -1e30f;
    }
    S6D_WAVE_RENDEZVOUS();   // (same-wave LDS order; on the GPU the wave's LDS operations execute in program order)
#pragma unroll
    for (int jt = 0; jt < 2; ++jt)
      *reinterpret_cast<float4 *>(tab + c * W16_LT + jt * 16 + g * 4) =
          make_float4(ah[jt][0] * kLog2e, ah[jt][1] * kLog2e, ah[jt][2] * kLog2e, ah[jt][3] * kLog2e);
    S6D_WAVE_RENDEZVOUS();   // (same-wave LDS order; on the GPU the wave's LDS operations execute in program order)
#pragma unroll
    for (int ky = 0; ky < SRC; ++ky) {
      const float v = tab[c * W16_LT + min(max(qy - ky + S - 1, 0), 31)];
      thv[n][ky] = ky < S ? v : -1e30f;
    }
    S6D_WAVE_RENDEZVOUS();   // (same-wave LDS order; on the GPU the wave's LDS operations execute in program order)
  }
}

// One pass of the row-padded window kernel: NS query rows against all key rows; the rows share every K / V
// fragment read.  A window holds at most 16 key rows, so a query row's whole score strip (SRC x 4 values per
// lane) stays in registers and the softmax is exact two-pass, not online:
//   A  S^T = K Q^T for every key row; s' = scale*acc + twr (one FMA), row maxima join a per-lane running max;
//   B  one cross-lane exchange for the strip maximum;
//   C  per 32-key step: P = exp2(s' - (m - thv)), then O^T += V^T P^T -- the V fragments of the step are requested
//      before the exponentials so their LDS latency hides under them, and the MFMAs of step u run under the
//      exponentials of step u+1.  The row sum comes from the matrix core too (an all-ones A fragment), so it is the
//      sum of the SAME bf16-rounded P that multiplies V and costs no VALU adds or lane exchanges.
// SRC = compile-time key-row count (even); EXACT: S == SRC (no unstaged key rows to skip).
struct Win16NoMid {
  __device__ __forceinline__ void operator()() const {}
};
// KROWT: K image row stride (elements); MID: called half way through the PV pass (the Q fragments are dead since the score pass,
// and by then half of the score registers are free).
template <int HD, int NS, int SRC, bool EXACT, int KROWT = Cfg<HD>::KROW, bool KSWZ = false, class MID = Win16NoMid>
__device__ __forceinline__ void win16_pass(const AttnParams &p, const u16 *Kl, const u16 *Vl, int S, int SR, int b,
                                           int wy, int wx, int head, int qy0, int rstride,
                                           const bf16x8 (&qf)[NS][Cfg<HD>::KS], const float (*twr)[4],
                                           const float (*thv)[16], int lane, MID mid = MID()) {
  using C = Cfg<HD>;
  const int g = lane >> 4, c = lane & 15;
  const int Cc = p.nh * HD;
  // ---- A: scores of every key row: S^T[key row ky][kx = g*4+r][query c] ----------------------------------
  float sp[NS][SRC][4], m[NS];
#pragma unroll
  for (int n = 0; n < NS; ++n) m[n] = -1e29f;                     // finite even if a whole strip is padding
  f32x4 cb[NS];
  {
    const float inv = 1.0f / p.scale_log2;
#pragma unroll
    for (int n = 0; n < NS; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) cb[n][r] = twr[n][r] * inv;          // masked columns: -1e30 / scale, still finite
  }
  bf16x8 kf[2][C::KS];
  // compact (LDS-DMA staged) images keep the chunk pairs of rows with (kx >> 2 ^ kx >> 3) & 1 swapped (kswz(); kx = c here)
  const int gk = KSWZ ? (g ^ kswz(c)) : g;
  auto kload = [&](int ky, bf16x8 (&dst)[C::KS]) {
    const int kyc = EXACT ? ky : min(ky, SR - 1);                   // rows >= SR are not staged: re-read a staged one
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks) {
      dst[ks] = *reinterpret_cast<const bf16x8 *>(Kl + (kyc * 16 + c) * KROWT + ks * 32 + gk * 8);
      // compact K rows (KROWT < padded head dim): the k range past HD is not staged -- the lane reads into the next row and
      // the fragment is zeroed here (the matching Q fragment is zero too, but 0 x a stray Inf would not be)
      if (KROWT < C::HDP && ks * 32 + 32 > HD && ks * 32 + g * 8 >= HD) {
        union { bf16x8 v; uint4 u; } z;
        z.u = make_uint4(0, 0, 0, 0);
        dst[ks] = z.v;
      }
    }
  };
  kload(0, kf[0]);
#pragma unroll
  for (int ky = 0; ky < SRC; ++ky) {
    if (ky + 1 < SRC) kload(ky + 1, kf[(ky + 1) & 1]);
    // the column bias rides the matrix core (round 5): the score chain starts from C = tw / scale_log2, so sp holds
    // (q.k + tw / scale) and the scale is applied inside the exponential's fma below -- one VALU instruction per score less
    f32x4 acc[NS];
#pragma unroll
    for (int n = 0; n < NS; ++n) acc[n] = cb[n];
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks)
#pragma unroll
      for (int n = 0; n < NS; ++n)
        acc[n] = S6D_ATTN_MFMA16(kf[ky & 1][ks], qf[n][ks], acc[n]);
#pragma unroll
    for (int n = 0; n < NS; ++n) {
#pragma unroll
      for (int r = 0; r < 4; ++r) sp[n][ky][r] = acc[n][r];
      const float mk = __builtin_fmaf(fmaxf(fmaxf(acc[n][0], acc[n][1]), fmaxf(acc[n][2], acc[n][3])), p.scale_log2, thv[n][ky]);
      m[n] = fmaxf(m[n], mk);
    }
  }
  // ---- B: strip maximum ----------------------------------------------------------------------------------------
#pragma unroll
  for (int n = 0; n < NS; ++n) {
    m[n] = fmaxf(m[n], __shfl_xor(m[n], 16));
    m[n] = fmaxf(m[n], __shfl_xor(m[n], 32));
  }
  // ---- C: P and O^T = V^T P^T over 32-key steps (key rows u, u+1) -------------------------------------------
  f32x4 oacc[NS][C::DT], lacc[NS];
#pragma unroll
  for (int n = 0; n < NS; ++n) {
    lacc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int dt = 0; dt < C::DT; ++dt) oacc[n][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  union { bf16x8 v; u16 hh[8]; } ones;
#pragma unroll
  for (int i = 0; i < 8; ++i) ones.hh[i] = S6D_ATTN_ONE;          // 1.0 in the element type
#pragma unroll
  for (int u = 0; u < SRC; u += 2) {
    // half of the score registers have been consumed: room for what `mid` brings in (the next item's Q fragments)
    if (u == ((SRC / 2 + 1) & ~1)) {
      __builtin_amdgcn_sched_barrier(0);                              // keep the loads `mid` issues from being hoisted into the first half
      mid();
      __builtin_amdgcn_sched_barrier(0);
    }
    if (EXACT || u < SR) {                                          // wave-uniform; K / V rows >= SR are not staged
      union { bf16x8 v; s16x4 q[2]; } va[C::DT];
      const u16 *vrow = Vl + (u * 16 + g * 4 + (c >> 2)) * C::VROW + (c & 3) * 4;
#pragma unroll
      for (int dt = 0; dt < C::DT; ++dt) {
        va[dt].q[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((S6D_LDS(s16x4) *)(vrow + dt * 16));
        va[dt].q[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((S6D_LDS(s16x4) *)(vrow + 16 * C::VROW + dt * 16));
      }
      union { bf16x8 v; u16 hh[8]; } pb[NS];
#pragma unroll
      for (int n = 0; n < NS; ++n)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const float nb = thv[n][u + h] - m[n];                    // m >= -1e29 (its initial value): a padded query's all-masked strip gives 0, not inf
          for (int r = 0; r < 4; ++r) pb[n].hh[h * 4 + r] = f2bf(fast_exp2(__builtin_fmaf(sp[n][u + h][r], p.scale_log2, nb)));
        }
#pragma unroll
      for (int n = 0; n < NS; ++n) lacc[n] = S6D_ATTN_MFMA16(ones.v, pb[n].v, lacc[n]);
#pragma unroll
      for (int dt = 0; dt < C::DT; ++dt)
#pragma unroll
        for (int n = 0; n < NS; ++n)
          oacc[n][dt] = S6D_ATTN_MFMA16(va[dt].v, pb[n].v, oacc[n][dt]);
    }
  }
#pragma unroll
  for (int n = 0; n < NS; ++n) {
    const int qy = qy0 + n * rstride;
    const int y = wy * p.ws + qy, x = wx * p.ws + c;
    if ((qy < S) && c < S && (y < p.H) && (x < p.W)) {
      const float inv = 1.0f / lacc[n][0];                          // every row of the ones-product is the strip's row sum
      u16 *dst = p.out + ((size_t)(b * p.H + y) * p.W + x) * (size_t)Cc + head * HD;
#pragma unroll
      for (int dt = 0; dt < C::DT; ++dt) {
        union { uint2 u2; u16 hh[4]; } o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o.hh[r] = f2bf(oacc[n][dt][r] * inv);
        *reinterpret_cast<uint2 *>(dst + dt * 16 + g * 4) = o.u2;
      }
    }
  }
}

// ---- round 5: the window pass as ONE stream, without the exact maximum -----------------------------------------------------
// win16_pass is exact two-pass softmax: all SRC x 4 scores of a strip stay in registers (112 for two strips of a 14 x 14 window)
// while the strip maximum is found, then the exponentials and P V run.  The maximum costs 1.25 vector instructions per score, the
// scale + bias another one, and the 112 registers put the kernel at the 256-VGPR limit.  As in process_tile_nomax (global
// attention): P only has to stay representable, bf16 has float32's exponent range, the accumulators are float32.  Here the reference
// value m is the maximum over the FIRST TWO key rows (32 of the 196 keys), known before the first exponential; every 32-key step then
// is score instructions -> exp2(fma(acc, scale_log2, th - m)) -> P V, nothing kept but the accumulators: 2.5 vector instructions
// per score instead of 4.75, no score array (182 VGPRs instead of 236).
// Safety net: a valid row whose sum is not < kNoMaxSumLimit = 2^100 (inf / NaN included) had scores more than ~92 log2 units above its reference
// (or its sum P V left float32: kNoMaxFinite); the
// WAVE then repeats the pass with that row's m raised by 96 (the sum drops by 2^96: any m within ~100 of the true maximum is as good
// as the maximum) until no row is out of range -- K / V stay resident in LDS for the whole item, so the retry is local to the wave,
// it is the same code (no second pass inlined: an exact-pass fallback pushed the kernel into scratch), and it terminates: scores
// of bf16 operands are finite, 40 rounds cover 3840 log2 units; NaN inputs give NaN outputs as they do in the exact pass.
// The column bias rides the matrix core (C = tw / scale_log2), masked columns carry -1e30 / scale there, a padded query's all-masked
// strip is clamped at m >= -1e29 so that its (discarded) P is 0, not inf.
// `next_q` is called once the last score instructions of the (first) round are issued: the caller loads the NEXT item's Q fragments
// into the registers of `qf`; `this_q` reloads THIS item's (before a retry round); after a retry `next_q` is called again at the end.
template <int HD, int SRC, int KROWT, bool KSWZ, class NEXTQ, class THISQ>
__device__ __forceinline__ void win16_pass_stream(const AttnParams &p, const u16 *Kl, const u16 *Vl, int S, int b, int wy, int wx,
                                                  int head, int qy0, int rstride, const bf16x8 (&qf)[2][Cfg<HD>::KS],
                                                  const float (*twr)[4], const float (*thv)[16], int lane, NEXTQ next_q, THISQ this_q) {
  using C = Cfg<HD>;
  constexpr int NS = 2;
  static_assert(SRC % 2 == 0 && SRC >= 4, "whole 32-key steps");
  const int g = lane >> 4, c = lane & 15;
  const int Cc = p.nh * HD;
  const int gk = KSWZ ? (g ^ kswz(c)) : g;
  f32x4 cb[NS];
  {
    const float inv = 1.0f / p.scale_log2;
#pragma unroll
    for (int n = 0; n < NS; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) cb[n][r] = twr[n][r] * inv;
  }
  bf16x8 kf[2][C::KS];
  auto kload = [&](int ky, bf16x8 (&dst)[C::KS]) __attribute__((always_inline)) {
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks) {
      dst[ks] = *reinterpret_cast<const bf16x8 *>(Kl + (ky * 16 + c) * KROWT + ks * 32 + gk * 8);
      if (KROWT < C::HDP && ks * 32 + 32 > HD && ks * 32 + g * 8 >= HD) {      // compact rows: the k range past HD reads into the next row
        union { bf16x8 v; uint4 u; } z;
        z.u = make_uint4(0, 0, 0, 0);
        dst[ks] = z.v;
      }
    }
  };
  auto scores = [&](const bf16x8 (&k)[C::KS], f32x4 (&acc)[NS]) __attribute__((always_inline)) {
#pragma unroll
    for (int n = 0; n < NS; ++n) acc[n] = cb[n];
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks)
#pragma unroll
      for (int n = 0; n < NS; ++n) acc[n] = S6D_ATTN_MFMA16(k[ks], qf[n][ks], acc[n]);
  };
  f32x4 s0[NS], s1[NS];
  kload(0, kf[0]);
  kload(1, kf[1]);
  scores(kf[0], s0);
  scores(kf[1], s1);
  float m[NS];
#pragma unroll
  for (int n = 0; n < NS; ++n) {
    const float m0 = __builtin_fmaf(fmaxf(fmaxf(s0[n][0], s0[n][1]), fmaxf(s0[n][2], s0[n][3])), p.scale_log2, thv[n][0]);
    const float m1 = __builtin_fmaf(fmaxf(fmaxf(s1[n][0], s1[n][1]), fmaxf(s1[n][2], s1[n][3])), p.scale_log2, thv[n][1]);
    float v = fmaxf(fmaxf(m0, m1), -1e29f);
    v = fmaxf(v, __shfl_xor(v, 16));
    v = fmaxf(v, __shfl_xor(v, 32));
    m[n] = v;
  }
  union { bf16x8 v; u16 hh[8]; } ones;
#pragma unroll
  for (int i = 0; i < 8; ++i) ones.hh[i] = S6D_ATTN_ONE;
  f32x4 oacc[NS][C::DT], lacc[NS];
  int round = 0;                                                      // wave-uniform
  for (;;) {
#pragma unroll
    for (int n = 0; n < NS; ++n) {
      lacc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int dt = 0; dt < C::DT; ++dt) oacc[n][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int u = 0; u < SRC; u += 2) {
      if (u > 0 || round > 0) {                                       // (round 0 enters with the first two rows' scores in s0 / s1)
        kload(u, kf[0]);
        kload(u + 1, kf[1]);
        scores(kf[0], s0);
        scores(kf[1], s1);
      }
      if (u == SRC - 2 && round == 0) {
        // the last score instructions are issued: the Q fragments are dead and the next item's go straight into their registers; the
        // last step's exponentials and P V, the end-of-item wait and the barrier cover the fetch
        __builtin_amdgcn_sched_barrier(0);
        next_q();
        __builtin_amdgcn_sched_barrier(0);
      }
      union { bf16x8 v; s16x4 q[2]; } va[C::DT];
      const u16 *vrow = Vl + (u * 16 + g * 4 + (c >> 2)) * C::VROW + (c & 3) * 4;
#pragma unroll
      for (int dt = 0; dt < C::DT; ++dt) {
        va[dt].q[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((S6D_LDS(s16x4) *)(vrow + dt * 16));
        va[dt].q[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((S6D_LDS(s16x4) *)(vrow + 16 * C::VROW + dt * 16));
      }
      union { bf16x8 v; u16 hh[8]; } pb[NS];
#pragma unroll
      for (int n = 0; n < NS; ++n) {
        const float nb0 = thv[n][u] - m[n], nb1 = thv[n][u + 1] - m[n];
        // (scalar FMAs on purpose: the packed form needs aligned register pairs and put this kernel into scratch)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          pb[n].hh[r] = f2bf(fast_exp2(__builtin_fmaf(s0[n][r], p.scale_log2, nb0)));
          pb[n].hh[4 + r] = f2bf(fast_exp2(__builtin_fmaf(s1[n][r], p.scale_log2, nb1)));
        }
      }
#pragma unroll
      for (int n = 0; n < NS; ++n) lacc[n] = S6D_ATTN_MFMA16(ones.v, pb[n].v, lacc[n]);
#pragma unroll
      for (int dt = 0; dt < C::DT; ++dt)
#pragma unroll
        for (int n = 0; n < NS; ++n) oacc[n][dt] = S6D_ATTN_MFMA16(va[dt].v, pb[n].v, oacc[n][dt]);
    }
    bool any_bad = false;
#pragma unroll
    for (int n = 0; n < NS; ++n) {
      const int qy = qy0 + n * rstride;
      int ovf = 0;                                                    // this lane's slice of the query's O^T column (4 g-lanes per query)
#pragma unroll
      for (int dt = 0; dt < C::DT; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) ovf |= !(fabsf(oacc[n][dt][r]) < kNoMaxFinite);
      ovf |= __shfl_xor(ovf, 16);
      ovf |= __shfl_xor(ovf, 32);
      const bool bad = (qy < S) && (c < S) && (!(lacc[n][0] < kNoMaxSumLimit) || ovf);     // a valid query's sum is >= 1 (its reference key)
      m[n] = bad ? m[n] + 96.0f : m[n];
      any_bad |= bad;
    }
    if (!__any(any_bad) || round >= 40) break;
    if (round == 0) this_q();                                         // this item's Q fragments again (next_q() replaced them)
    ++round;
  }
  if (round > 0) next_q();
#pragma unroll
  for (int n = 0; n < NS; ++n) {
    const int qy = qy0 + n * rstride;
    const int y = wy * p.ws + qy, x = wx * p.ws + c;
    if ((qy < S) && c < S && (y < p.H) && (x < p.W)) {
      const float inv = 1.0f / lacc[n][0];
      u16 *dst = p.out + ((size_t)(b * p.H + y) * p.W + x) * (size_t)Cc + head * HD;
#pragma unroll
      for (int dt = 0; dt < C::DT; ++dt) {
        union { uint2 u2; u16 hh[4]; } o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o.hh[r] = f2bf(oacc[n][dt][r] * inv);
        *reinterpret_cast<uint2 *>(dst + dt * 16 + g * 4) = o.u2;
      }
    }
  }
}

// ---- windowed, row-padded (S <= 16): key slot = ky*16 + kx, so every 16-key MFMA sub-tile is ONE key row and
// every 16-query strip is ONE query row: the decomposed bias costs one LDS word per sub-tile (rel_h) plus four
// registers (rel_w, kx = g*4+r fixed per lane; out-of-window columns carry -1e30 there, which is the mask).
template <int HD, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void attn_window16_kernel(AttnParams p) {
  using C = Cfg<HD>;
  S6D_DYN_LDS(smem);
  const int S = p.S, SR = (S + 1) & ~1;                            // key rows, rounded up to a 32-key k-step
  u16 *Kl = reinterpret_cast<u16 *>(smem);                         // [SR*16][KROW]
  u16 *Vl = Kl + (size_t)SR * 16 * C::KROW;                        // [SR*16][VROW]
  float *tabs = reinterpret_cast<float *>(Vl + (size_t)SR * 16 * C::VROW);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int g = lane >> 4, c = lane & 15;
  float *tab = tabs + (size_t)wave * 16 * W16_LT;                 // one [16][W16_LT] scratch table per wave

  WinItem item;
  item.decode(p, blockIdx.x);
  const int head = item.head, wx = item.wx, wy = item.wy, b = item.b;
  const int Cc = p.nh * HD;
  // Q fragments of every query row this wave owns are fetched first so their latency hides under the staging
  constexpr int MAXROWS = 2;                                      // rows (wave, wave + WAVES); WAVES >= 8 covers S <= 16
  static_assert(2 * WAVES >= 16, "two rows per wave must cover 16 query rows");
  bf16x8 qfa[MAXROWS][C::KS];
#pragma unroll
  for (int i = 0; i < MAXROWS; ++i) {
    const int qy = wave + i * WAVES;
    const int y = wy * p.ws + qy, x = wx * p.ws + c;
    const bool qwin = c < S && qy < S, qimg = qwin && (y < p.H) && (x < p.W);
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks) {
      union { uint4 u; bf16x8 v; } t;
      const int d0 = ks * 32 + g * 8;
      const int dc = d0 < HD ? d0 : HD - 8;
      const size_t tokc = (size_t)(b * p.H + min(y, p.H - 1)) * p.W + min(x, p.W - 1);
      const u16 *src = qimg ? qkv_at(p, tokc, 0, head) + dc : p.qkv_bias + head * HD + dc;
      t.u = *reinterpret_cast<const uint4 *>(src);
      if (!(qwin && d0 < HD)) t.u = make_uint4(0, 0, 0, 0);
      qfa[i][ks] = t.v;
    }
  }
  RelFrags<HD> rf;
  rf.load(p, lane);
  // stage K and V of the whole window (bias vector for out-of-image slots, zeros for padding slots): UN
  // independent 16-byte loads per thread are in flight before any is written to LDS, and the first batch
  // flies under the bias-table MFMAs (which need only Q and the position tables).
  constexpr int UN = 10;
  const int total = SR * 16 * (C::KPARTS + C::VPARTS);
  uint4 sv[UN];
  u16 *sdst[UN];
  auto issue = [&](int i0) {
#pragma unroll
    for (int n = 0; n < UN; ++n) {
      const int i = i0 + n * WAVES * 64;
      const int iq = min(i, total - 1);
      const bool isv = iq >= SR * 16 * C::KPARTS;
      const int ii = isv ? iq - SR * 16 * C::KPARTS : iq;
      const int parts = isv ? C::VPARTS : C::KPARTS;
      const int slot = ii / parts, part = ii - slot * parts;
      const int ky = slot >> 4, kx = slot & 15;
      const int y = wy * p.ws + ky, x = wx * p.ws + kx;
      sdst[n] = (i < total) ? (isv ? Vl + slot * C::VROW + part * 8 : Kl + slot * C::KROW + part * 8) : nullptr;
      const bool img = (y < p.H) && (x < p.W);
      const int dc = part * 8 < HD ? part * 8 : HD - 8;
      const size_t tokc = (size_t)(b * p.H + min(y, p.H - 1)) * p.W + min(x, p.W - 1);
      const int sel = (isv ? 2 : 1) * Cc + head * HD + dc;
      const u16 *src = img ? qkv_at(p, tokc, isv ? 2 : 1, head) + dc : p.qkv_bias + sel;
      sv[n] = *reinterpret_cast<const uint4 *>(src);
      if (!(ky < S && kx < S && part * 8 < HD)) sv[n] = make_uint4(0, 0, 0, 0);
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int n = 0; n < UN; ++n)
      if (sdst[n]) *reinterpret_cast<uint4 *>(sdst[n]) = sv[n];
  };
  const bool stage = !(kAbl & 1);
  if (stage) issue(tid);
  // bias registers; tables are instantiated for the key-row count the pass will use
  float twr[MAXROWS][4], thv[MAXROWS][16];
  if (!(kAbl & 2)) {
    if (S > WAVES) {
      if (S == 14)
        win16_tables<HD, 2, 14>(rf, S, wave, WAVES, qfa, tab, twr, thv, lane);
      else
        win16_tables<HD, 2, 16>(rf, S, wave, WAVES, qfa, tab, twr, thv, lane);
    } else if (wave < S) {
      win16_tables<HD, 1, 8>(rf, S, wave, WAVES, qfa, tab, twr, thv, lane);
    }
  }
  if (stage) {
    commit();
    for (int i0 = tid + UN * WAVES * 64; i0 < total; i0 += UN * WAVES * 64) {
      issue(i0);
      commit();
    }
  }
  __syncthreads();

  // S <= WAVES: one query row per wave; otherwise two rows per wave share every K / V fragment read:
  // rows (wave, wave + WAVES).
  if (S <= WAVES) {
    if (wave < S && !(kAbl & 2)) {
      const bf16x8 (&q1)[1][C::KS] = reinterpret_cast<const bf16x8 (&)[1][C::KS]>(qfa[0]);
      win16_pass<HD, 1, 8, false>(p, Kl, Vl, S, SR, b, wy, wx, head, wave, WAVES, q1, twr, thv, lane);
    }
  } else if (!(kAbl & 2)) {
    static_assert(MAXROWS >= 2 || WAVES >= 16, "row bookkeeping");
    const bf16x8 (&q2)[2][C::KS] = reinterpret_cast<const bf16x8 (&)[2][C::KS]>(qfa[0]);
    if (S == 14) {
      win16_pass<HD, 2, 14, true>(p, Kl, Vl, S, SR, b, wy, wx, head, wave, WAVES, q2, twr, thv, lane);
    } else
      win16_pass<HD, 2, 16, false>(p, Kl, Vl, S, SR, b, wy, wx, head, wave, WAVES, q2, twr, thv, lane);
  }
}

// ---- windowed, row-padded, PERSISTENT: one 8-wave workgroup per CU walks its share of the (window, head) items; the K / V
// images of item i + 1 arrive by LDS-DMA into the second half of LDS while item i is computed from the first.
//
// Why: the one-item-per-workgroup kernel above spends an item as [fetch 107 KB | arithmetic | store]: with one 98-KiB workgroup
// per CU nothing overlaps, and the CU's fetch path (~10 B/clk/CU from HBM, MI355X_MICROARCH.md) is idle for half of the item.
// Two smaller workgroups per CU did not help (each needs its own copy of the window: 0.375 vs 0.358 ms per 16 frames); keeping
// the fetch path busy does -- a register-free prefetch of the NEXT item, which LDS-DMA provides.
//   * LDS (all 160 KiB): 2 x [K image 224 slots x 11 chunks (10 data + 1 pad: 176-B rows are bank-conflict free for the fragment
//     reads) padded to 39 KiB | V image 224 x 10 chunks = 35 KiB] + the two padded rel-pos tables (12 KiB, read as A fragments per
//     item instead of being held in 48 VGPRs across the loop).  The per-wave scratch tables of win16_tables live in the V area
//     of the buffer that is being FILLED: the K image of the next item goes out first, the V image after the tables are done.
//   * an image is lane-linear for the DMA (64 consecutive 16-byte chunks per instruction); the lane works out which (slot, part)
//     its chunk is: in-window in-image -> the token's k / v run, out-of-image -> the qkv bias (quirk Q2 of SURVEY: padded tokens
//     carry the bias), outside the 14 x 14 window or the pad chunk -> a 16-byte zero in global memory.
//   * Q fragments of item i + 1 are loaded into the registers of item i's Q fragments half way through item i's PV pass (they are
//     dead since the score pass, and half of the score registers are free by then).
// Measured (16 frames, 6400 items): 0.305 ms against 0.350 ms for the one-item kernel (profiles/r02_win16_variants.txt).  Tried on
// top and dropped, both slower: keeping the packed output rows in registers and storing them after the end-of-item wait (so that the
// wait does not cover the stores): 0.396 ms; that plus folding the row bias into the scores to free 28 registers in the PV pass:
// 0.431 ms (the kernel sits at the 256-VGPR limit: every extra live value in the PV pass became scratch traffic in the hot loop).

// S14: the kernel is instantiated once for 14 x 14 windows (the ViT-H configuration: every key row exists, win16_pass<.., 14, true>)
// and once for the other sizes (win16_pass<.., 16, false>).  As ONE kernel holding both passes it needed 256 VGPRs + 21 spilled
// registers, stored to scratch for every item on either path; the 14 x 14 instantiation alone takes 239 VGPRs and no scratch
// (round 4: tools/kernel_resources.py).
template <int HD, bool S14>
__global__ __launch_bounds__(512) void attn_window16p_kernel(AttnParams p, int nitems) {
  using C = Cfg<HD>;
  constexpr int WAVES = 8;
  constexpr int KROWT = HD + 8, KCH = KROWT / 8, VCH = C::VROW / 8;   // chunks (16 B) per K / V row
  S6D_DYN_LDS(smem);
  const int S = p.S, SR = (S + 1) & ~1;
  const int kchunks = SR * 16 * KCH, vchunks = SR * 16 * VCH;
  const int kinstr = (kchunks + 63) >> 6, vinstr = (vchunks + 63) >> 6;
  const int kbytes = kinstr << 10, bufbytes = kbytes + (vinstr << 10);
  u16 *relh = reinterpret_cast<u16 *>(smem + 2 * bufbytes);        // [32][HDP] padded rel_pos_h, then rel_pos_w
  u16 *relw = relh + 32 * C::HDP;
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int g = lane >> 4, c = lane & 15;
  const int Cc = p.nh * HD;
  // rel tables -> LDS, once.  A row is HDP / 8 = 12 (8) chunks of 16 bytes, so the 16 rows of a fragment read start on only 4 (2) of
  // the 16 bank slots: every one of the 12 fragment reads per item was a 4-way conflict -- 2.3 k of a workgroup's ~28 k cycles per
  // item, and the whole of the kernel's SQ_LDS_BANK_CONFLICT count (14.5 M per launch = 6400 items x 2.3 k, profiles/r04_sq_summary
  // .json).  There is no LDS left for padded rows (2 x 74 KiB images + 12 KiB tables = 160 KiB), so the chunks of
  // row r are stored at chunk ^ ((r >> 2) & 3): inside a group of four chunks, 16 rows x one chunk index -> 16 distinct slots.
  constexpr int RCH = C::HDP / 8;
  for (int i = tid; i < 2 * 32 * RCH; i += 512) {
    const bool w = i >= 32 * RCH;
    const int ii = w ? i - 32 * RCH : i;
    const int row = ii / RCH, ch = ii - row * RCH;
    reinterpret_cast<uint4 *>(w ? relw : relh)[row * RCH + (ch ^ ((row >> 2) & 3))] = reinterpret_cast<const uint4 *>(w ? p.rel_w : p.rel_h)[ii];
  }

  // ---- DMA of one image: `which` 1 = K (row KCH chunks, the last one padding), 2 = V.
  // Which chunk of the image a lane feeds in the wave's i-th DMA instruction -- key row, key column, head-dim part, inside the
  // S x S window or not -- does not depend on the item: it is computed ONCE per kernel and kept packed in one register per
  // instruction slot (round 5).  Until then every instruction recomputed it (a division by the row's chunk count, the swizzle, two
  // 64-bit token products: ~56 instructions per DMA instruction, ~10 per wave and item: a quarter of the wave's instruction
  // stream).  Per item only the window origin, the image test at the frame's edge and one 64-bit multiply-add remain.
  constexpr int MAXI = S14 ? 5 : 6;                                  // DMA instructions per wave and image: ceil(14 (16) x 16 x 11 / 64 / 8)
  // the slots are unrolled: an image with more 1-KiB pieces than WAVES x MAXI would silently lose its tail -- the
  // largest window this instantiation serves (14 rows, or 16 = the launcher's limit) must fit for both images
  static_assert(((S14 ? 14 : 16) * 16 * (KCH > VCH ? KCH : VCH) + 63) / 64 <= WAVES * MAXI,
                "attn_window16p_kernel: K / V image has more DMA pieces than the unrolled slots (raise MAXI)");
  unsigned kvc[MAXI];                     // per instruction slot: K in bits 0-12, V in bits 16-28: ky | kx << 4 | part << 8 | inwin << 12
  {
#pragma unroll
    for (int i = 0; i < MAXI; ++i) {
      unsigned both = 0;
#pragma unroll
      for (int which = 1; which <= 2; ++which) {
        const int rowch = which == 1 ? KCH : VCH, nch = which == 1 ? kchunks : vchunks;
        const int k = wave + i * WAVES;
        const int j = min((k << 6) + lane, nch - 1);                  // chunk of the image (tail lanes repeat the last chunk's source)
        const int slot = j / rowch, pp = j - slot * rowch;
        const int ky = slot >> 4, kx = slot & 15;
        const int part = (S6D_WIN16_KSWZ && which == 1 && pp * 8 < HD) ? pp ^ kswz(kx) : pp;     // K: chunk pairs swapped on the source side
        const bool inwin = ky < S && kx < S && part * 8 < HD;
        const unsigned v = (unsigned)(ky & 15) | ((unsigned)kx << 4) | ((unsigned)part << 8) | ((unsigned)inwin << 12);
        both |= which == 1 ? v : v << 16;
      }
      kvc[i] = both;
    }
  }
  auto stage_image = [&](const WinItem &it, int which, char *dst_base) __attribute__((always_inline)) {
    const int ninstr = which == 1 ? kinstr : vinstr;
    const int y0 = it.wy * p.ws, x0 = it.wx * p.ws, bH = it.b * p.H;
    const u16 *base = qkv_at(p, 0, which, it.head);                   // wave-uniform
    const u16 *bias_base = p.qkv_bias + which * Cc + it.head * HD;
#pragma unroll
    for (int i = 0; i < MAXI; ++i) {
      const int k = wave + i * WAVES;
      if (k < ninstr) {                                               // wave-uniform
        unsigned cc = which == 1 ? kvc[i] : kvc[i] >> 16;
        S6D_PIN(cc);                        // opaque per item: the unpacked fields must not be hoisted out of the item loop (40 registers)
        const int ky = (int)(cc & 15u), kx = (int)((cc >> 4) & 15u), po = min((int)((cc >> 8) & 15u) * 8, HD - 8);
        const int y = y0 + ky, x = x0 + kx;
        const bool img = (y < p.H) && (x < p.W);
        const unsigned tok = (unsigned)(bH + min(y, p.H - 1)) * (unsigned)p.W + (unsigned)min(x, p.W - 1);
        const u16 *s_img = base + (size_t)tok * (size_t)p.tok_stride + po;
        const u16 *src = img ? s_img : bias_base + po;
        const void *sp = (cc >> 12) & 1u ? (const void *)src : (const void *)&g_attn_zero16;
        S6D_LDS(char) *dst = (S6D_LDS(char) *)dst_base + (k << 10);
        lds_dma16_m0(sp, dst);                 // (the inline-asm issue, so that the prefetch overlaps the arithmetic: csrc/s6d_mem.h)
      }
    }
  };
  constexpr int MAXROWS = 2;
  bf16x8 qfa[MAXROWS][C::KS];
  // RAW: loads only (the zero mask of the out-of-window / padded-head-dim chunks is lane-constant and applied by mask_q at the
  // start of the item that uses the fragments, behind the end-of-item wait)
  auto load_q = [&](const WinItem &it, bool raw, bf16x8 (&qdst)[MAXROWS][C::KS]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < MAXROWS; ++i) {
      const int qy = wave + i * WAVES;
      const int y = it.wy * p.ws + qy, x = it.wx * p.ws + c;
      const bool qwin = c < S && qy < S, qimg = qwin && (y < p.H) && (x < p.W);
#pragma unroll
      for (int ks = 0; ks < C::KS; ++ks) {
        union { uint4 u; bf16x8 v; } t;
        const int d0 = ks * 32 + g * 8;
        const int dc = d0 < HD ? d0 : HD - 8;
        const size_t tokc = (size_t)(it.b * p.H + min(y, p.H - 1)) * p.W + min(x, p.W - 1);
        const u16 *src = qimg ? qkv_at(p, tokc, 0, it.head) + dc : p.qkv_bias + it.head * HD + dc;
        t.u = *reinterpret_cast<const uint4 *>(src);
        if (!raw && !(qwin && d0 < HD)) t.u = make_uint4(0, 0, 0, 0);
        qdst[i][ks] = t.v;
      }
    }
  };
  auto mask_q = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < MAXROWS; ++i) {
      const bool qwin = c < S && wave + i * WAVES < S;
#pragma unroll
      for (int ks = 0; ks < C::KS; ++ks) {
        union { uint4 u; bf16x8 v; } t;
        t.v = qfa[i][ks];
        if (!(qwin && ks * 32 + g * 8 < HD)) t.u = make_uint4(0, 0, 0, 0);
        qfa[i][ks] = t.v;
      }
    }
  };

  WinItem cur, nxt;
  int id = blockIdx.x;
  cur.decode(p, id);
  load_q(cur, false, qfa);
  stage_image(cur, 1, smem);
  stage_image(cur, 2, smem + kbytes);
  S6D_VMCNT(0);
  __syncthreads();
  int buf = 0;
  long long wtk[8] = {0, 0, 0, 0, 0, 0, 0, 0}, wsum[6] = {0, 0, 0, 0, 0, 0};   // S6D_G64_TIMING probe build: phase clocks, see below
  for (; id < nitems; id += gridDim.x) {
    char *cb = smem + buf * bufbytes, *nb = smem + (buf ^ 1) * bufbytes;
    const bool more = id + (int)gridDim.x < nitems;
    S6D_TICK(wtk, 0);
    if (more) {
      nxt.decode(p, id + gridDim.x);
      stage_image(nxt, 1, nb);                                       // K image of the next item; its V area is this item's scratch
    }
    // bias registers of this item (rel-pos tables as A fragments from LDS; scratch tables in the V area of the other buffer)
    float twr[MAXROWS][4], thv[MAXROWS][16];
    {
      RelFrags<HD> rf;
#pragma unroll
      for (int jt = 0; jt < 2; ++jt)
#pragma unroll
        for (int ks = 0; ks < C::KS; ++ks) {
          const int ro = (jt * 16 + c) * C::HDP + ((ks * 4 + g) ^ (((jt * 16 + c) >> 2) & 3)) * 8;     // chunk swizzle of the copy above
          rf.rh[jt][ks].u = *reinterpret_cast<const uint4 *>(relh + ro);
          rf.rw[jt][ks].u = *reinterpret_cast<const uint4 *>(relw + ro);
        }
      float *tab = reinterpret_cast<float *>(nb + kbytes) + (size_t)wave * 16 * W16_LT;
      if (S == 14)
        win16_tables<HD, 2, 14>(rf, S, wave, WAVES, qfa, tab, twr, thv, lane);
      else
        win16_tables<HD, 2, 16>(rf, S, wave, WAVES, qfa, tab, twr, thv, lane);
    }
    S6D_TICK(wtk, 1);
    __builtin_amdgcn_s_barrier();                                    // every wave is done with its scratch table (raw: the K DMA stays in flight)
    S6D_TICK(wtk, 2);
    if (more) stage_image(nxt, 2, nb + kbytes);
    S6D_TICK(wtk, 3);
    const u16 *Kl = reinterpret_cast<const u16 *>(cb), *Vl = reinterpret_cast<const u16 *>(cb + kbytes);
    const bf16x8 (&q2)[2][C::KS] = reinterpret_cast<const bf16x8 (&)[2][C::KS]>(qfa[0]);
    if (S14 && S6D_WIN16_STREAM) {
      // the streaming pass keeps this item's Q fragments live to its last score instructions; the next item's are requested right
      // there, into the same registers (a retry round of the pass fetches this item's again)
      auto next_q = [&]() __attribute__((always_inline)) {
        if (more) load_q(nxt, true, qfa);
      };
      auto this_q = [&]() __attribute__((always_inline)) { load_q(cur, false, qfa); };
      win16_pass_stream<HD, 14, KROWT, S6D_WIN16_KSWZ != 0>(p, Kl, Vl, S, cur.b, cur.wy, cur.wx, cur.head, wave, WAVES, q2, twr, thv, lane,
                                                            next_q, this_q);
    } else {
      auto mid = [&]() __attribute__((always_inline)) {              // half way through the PV pass: this item's Q fragments are long dead
        if (more) load_q(nxt, true, qfa);
      };
      if (S14)
        win16_pass<HD, 2, 14, true, KROWT, S6D_WIN16_KSWZ != 0>(p, Kl, Vl, S, SR, cur.b, cur.wy, cur.wx, cur.head, wave, WAVES, q2, twr, thv, lane, mid);
      else
        win16_pass<HD, 2, 16, false, KROWT, S6D_WIN16_KSWZ != 0>(p, Kl, Vl, S, SR, cur.b, cur.wy, cur.wx, cur.head, wave, WAVES, q2, twr, thv, lane, mid);
    }
    S6D_TICK(wtk, 4);
    S6D_VMCNT(0);                                                  // next item's images and Q have landed (and this item's stores)
    S6D_TICK(wtk, 5);
    __syncthreads();
    S6D_TICK(wtk, 6);
    if (S6D_G64_TIMING)
#pragma unroll
      for (int i = 0; i < 6; ++i) wsum[i] += wtk[i + 1] - wtk[i];
    // unconditional: on the last item the fragments are stale and unused, but hipcc's wait-count model then sees every path into the
    // loop header with no load in flight (otherwise it waits vmcnt(5..0) at the fragments' first use, i.e. for the K DMA issued before it)
    // (The alternative was to mask the next item's Q fragments right behind their loads, a full fetch latency inside the PV pass:
    // docs/NOTEBOOK_r1_r4.md section 4.2, profiles/r04_win16_dma_waits.txt.)
    mask_q();
    cur = nxt;
    buf ^= 1;
  }
  // probe build: [K DMA issue + bias tables | barrier | V DMA issue | score / softmax / P V passes | vmcnt(0) | barrier] per wave of
  // workgroup 8, 320 bytes behind the output tensor (tools/attn_time.py)
  if (S6D_G64_TIMING && blockIdx.x == 8 && lane == 0) {
    long long *dbg = reinterpret_cast<long long *>(p.out + (size_t)p.B * p.H * p.W * p.nh * HD);
#pragma unroll
    for (int i = 0; i < 6; ++i) dbg[wave * 6 + i] = wsum[i];
  }
}

template <int HD>
static int launch_win16(AttnParams p, hipStream_t st) {
  using C = Cfg<HD>;
  constexpr int WAVES = 8;                                      // rows (wave, wave + 8): two query rows per wave share every
                                                                // K / V fragment read (measured: 8x2 rows 0.23 ms vs 14x1 rows 0.25 ms per 8 frames)
  const int SR = (p.S + 1) & ~1;
  // persistent, LDS-DMA double-buffered kernel: two query rows per wave (S > 8), both images + the rel tables inside 160 KiB;
  // windows of up to 8 rows take the one-item kernel below
  if (p.S > WAVES) {
    const int kin = (SR * 16 * (HD + 8) / 8 + 63) / 64, vin = (SR * 16 * C::VROW / 8 + 63) / 64;
    const size_t lds = (size_t)2 * (kin + vin) * 1024 + (size_t)2 * 32 * C::HDP * 2;
    const int nitems = p.B * p.nwy * p.nwx * p.nh;
    if (lds <= 160 * 1024 && (size_t)WAVES * 16 * W16_LT * 4 <= (size_t)vin * 1024) {
      int grid = nitems < 256 ? nitems : 256;                   // one persistent workgroup per CU
      if (s6d::g_s6d_persistent_grid_limit > 0 && s6d::g_s6d_persistent_grid_limit < grid) grid = s6d::g_s6d_persistent_grid_limit;   // set through the ABI (tests)
      if (grid >= 8) grid &= ~7;                                // whole XCD rounds: workgroup j keeps to XCD j % 8, like its items
      if (p.S == 14) {
        launch_lds(attn_window16p_kernel<HD, true>, grid, 512, lds, st, p, nitems);
      } else {
        launch_lds(attn_window16p_kernel<HD, false>, grid, 512, lds, st, p, nitems);
      }
      return launch_status();
    }
  }
  const size_t lds = (size_t)SR * 16 * (C::KROW + C::VROW) * 2 + (size_t)WAVES * 16 * W16_LT * 4;
  if (lds > 160 * 1024) return S6D_EUNSUPPORTED;
  launch_lds(attn_window16_kernel<HD, WAVES>, (unsigned)(p.B * p.nwy * p.nwx * p.nh), WAVES * 64, lds, st, p);
  return launch_status();
}

}  // namespace S6D_ATTN_NS
