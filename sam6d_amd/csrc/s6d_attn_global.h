// Global attention over the whole H x W grid (T % 64 == 0): attn_global_kernel streams K / V tiles through registers into a 2-deep LDS
// ring (any grid; table bias or none), attn_global64_kernel is the LDS-DMA kernel of the 64 x 64 grid (ViT-H's four global blocks).
#pragma once
#include "s6d_attn_common.h"

namespace S6D_ATTN_NS {

// s_setprio 1 around the MFMA phases of a process_tile (the wave in its MFMA phase wins issue over the one in softmax).  The
// alternative was no priority change (S6D_GLB_PRIO = 0): profiles/r02_attn_variants.txt (`prio`, `noprio`).
constexpr bool kGlbPrio = true;

// ---- global: one workgroup per (image, head, 128-query tile); KV tiles stream through a 2-deep LDS ring -----
// Each wave owns NS = 2 strips (32 queries): K/V fragments and every staged tile are shared by twice the math.
template <int HD, int WAVES, int MODE>
__global__ __launch_bounds__(WAVES * 64) void attn_global_kernel(AttnParams p) {
  using C = Cfg<HD>;
  constexpr int NS = 2;
  // MODE 1 (the aligned 64 x 64 fast path, th tables at a 65-float row stride: S6D_GLB_THLD) ran here until attn_global64_kernel took
  // that grid (docs/NOTEBOOK_r1_r4.md section 4.2, profiles/r02_attn_variants.txt)
  static_assert(MODE == 0 || MODE == 2, "attn_global_kernel: table bias (0) or no bias (2); the 64 x 64 grid is attn_global64_kernel's");
  S6D_DYN_LDS(smem);
  constexpr int KBYTES = 64 * C::KROW * 2, VBYTES = 64 * C::VROW * 2;
  // ring slot r: K image at r*(KBYTES+VBYTES), V image right behind it
  auto Kbuf = [&](int r) { return reinterpret_cast<u16 *>(smem + r * (KBYTES + VBYTES)); };
  auto Vbuf = [&](int r) { return reinterpret_cast<u16 *>(smem + r * (KBYTES + VBYTES) + KBYTES); };
  float *tabs = reinterpret_cast<float *>(smem + 2 * (KBYTES + VBYTES));
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c = lane & 15;

  // Workgroup -> (image, head, query tile).  All query tiles of one (image, head) re-read the same 1.3 MB of
  // K/V: keep them on ONE XCD (observed placement: block id % 8) so the re-reads hit that XCD's 4 MB L2
  // instead of streaming from HBM once per query tile.  Pure speed choice; any placement is correct.
  const int nqt = (p.T + WAVES * 16 * NS - 1) / (WAVES * 16 * NS);
  int id = blockIdx.x;
  const int nbh = p.B * p.nh;
  int qt, bh;
  if ((nbh & 7) == 0) {
    const int xcd = id & 7, loc = id >> 3;
    qt = loc % nqt;
    bh = (loc / nqt) * 8 + xcd;
  } else {
    qt = id % nqt;
    bh = id / nqt;
  }
  const int head = bh % p.nh, b = bh / p.nh;
  StripState<HD, NS> st;
  int q0[NS];
#pragma unroll
  for (int n = 0; n < NS; ++n) {
    q0[n] = ((qt * WAVES + wave) * NS + n) * 16;
    load_q<HD>(p, b, 0, 0, head, q0[n], st.qf[n], lane);
    const int qi = min(q0[n] + c, p.T - 1);
    st.qy[n] = div_S(p, qi);
    st.qx[n] = qi - st.qy[n] * p.S;
    st.m_run[n] = -1e30f;
    st.lacc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 16; ++i) st.twr[n][i] = 0.f;
#pragma unroll
    for (int dt = 0; dt < C::DT; ++dt) st.oacc[n][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    st.th[n] = nullptr;
    st.tw[n] = nullptr;
  }
  if (MODE == 0) {
#pragma unroll
    for (int n = 0; n < NS; ++n) {
      float *th = tabs + (size_t)(wave * NS + n) * 2 * 16 * p.LT, *tw = th + 16 * p.LT;
      for (int jt = 0; jt < p.LT / 16; ++jt) {
        build_table<HD, 1>(p.rel_h, jt * 16, 1, st.qf[n], th + jt * 16, p.LT, lane);
        build_table<HD, 1>(p.rel_w, jt * 16, 1, st.qf[n], tw + jt * 16, p.LT, lane);
      }
      st.th[n] = th;
      st.tw[n] = tw;
    }
  }
  const int ntile = p.T / 64;                       // launcher guarantees T % 64 == 0 for this kernel
  StagerLinear<HD, WAVES * 64> sg;
  sg.init(p, b, head, tid);
  const size_t tstride = (size_t)64 * (size_t)p.tok_stride;
  sg.load(tstride, 0);
  __syncthreads();                                  // table scratch (aliasing the ring) fully consumed
  sg.store(Kbuf(0));
  __syncthreads();
  auto tile = [&](int t) {
    const float thv[NS] = {0.f, 0.f};
    if (!(kAbl & 2)) process_tile<HD, MODE, NS, true, kGlbPrio>(p, Kbuf(t & 1), Vbuf(t & 1), t * 64, st, thv, lane);
  };
  for (int t = 0; t + 1 < ntile; ++t) {                           // steady state: branch-free body
    if (!(kAbl & 1)) sg.load(tstride, t + 1);                     // flies under this tile's math
    tile(t);
    if (!(kAbl & 32)) sg.store(Kbuf((t & 1) ^ 1));                // ring slot last read in iteration t-1
    __syncthreads();
  }
  tile(ntile - 1);
#pragma unroll
  for (int n = 0; n < NS; ++n) store_strip<HD>(p, b, 0, 0, head, q0[n], st.lacc[n][0], st.oacc[n], lane);
}

// ---- global over the 64 x 64 grid, LDS-DMA staged: 8 waves x 32 queries per workgroup, K / V tiles through a 3-slot ring -------
// What the kernel above pays for besides its arithmetic (16 frames x 16 heads, same process, profiles/r02_attn_variants.txt):
// 2.22 ms as is, 1.75 ms without the staging of K / V tiles, 1.30 ms for the staging ALONE -- every 128-query workgroup pulls all
// 1.3 MB of its head's K and V through registers into LDS, one tile of look-ahead, 6 loads + 6 ds_write_b128 per thread and tile.
// Here: 256 queries per workgroup (half the K / V passes), tiles DMA'd straight into LDS (global_load_lds, 3 instructions per
// wave and tile, no staging registers, no ds_write) two tiles ahead of the arithmetic behind counted vmcnt waits and ONE raw
// s_barrier per tile, K rows chunk-swizzled on the source address (kswz(): conflict-free fragment reads), th tables
// at a 65-float row stride.  A ring slot is [K image 64 rows x (HDP + 8) | V image 64 x VROW]; every wave issues the same number
// of DMA instructions per tile (3 with 8 waves), so one vmcnt(3) means "my pieces of this tile landed".
// Measured in one process (16 frames, min of 3 x 20 launches): 1.73 ms (795 TFLOP/s) against 1.89 ms for the round-1 kernel,
// 1.81 ms for it with the two layout switches, 1.78 ms for it with 8 waves; 4 waves + 2 slots here: 1.77 ms.
// Where the rest goes (phase clocks of S6D_G64_TIMING, per tile and wave, older / younger half of the workgroup): barrier wait
// 850 / 180, DMA issue + th read 190 / 370, QK^T + scale + max 1260 / 1370, exp + pack 515 / 915, P V 545 / 530 -- about 3400
// cycles per tile for 96 MFMAs (1536 matrix-pipe cycles) and 2 x 158 VALU instructions on each SIMD.  The issue-rate probe
// (tools/probes/valu_rate.hip, profiles/r02_valu_rate.txt) says why: with two or more waves on a SIMD, MFMA and VALU issue time ADD
// (8 MFMA 57 ns, 48 v_fma 55 ns, 8 x (MFMA, 6 v_fma) 109 ns per wave; v_exp_f32 = 3 v_fma, packed fp32 ops = 1.8), so the
// softmax's 3.3 VALU instructions per MFMA cost about as much as the MFMAs themselves.  Tried on this kernel and dropped (no
// gain, same process): the tile as ONE interleaved stream -- K fragments read two 16-key blocks ahead, block i's scale / max
// beside block i + 1's MFMAs, P of keys 0..31 exponentiated speculatively against the old maximum beside the QK^T MFMAs, P of
// keys 32..63 beside the first P V MFMAs (1.74 ms, bit-identical output); static s_setprio 1 for the younger half (1.75 ms);
// rings of 2 and (without the th tables, as a timing probe) 6 slots (1.69 - 1.75 ms: the look-ahead is not what is missing).
constexpr int G64_THLD = 65;
#ifndef S6D_G64_SLOTS
#define S6D_G64_SLOTS 3             // ring depth: tiles are DMA'd S6D_G64_SLOTS - 1 ahead of the arithmetic
#endif
#ifndef S6D_G64_WAVES
#define S6D_G64_WAVES 8
#endif
#ifndef S6D_G64_NOMAX
#define S6D_G64_NOMAX 1             // tiles after the first without a running maximum (process_tile_nomax); 0: round-4 arithmetic
#endif

template <int HD, int WAVES_, int SLOTS_>
struct G64 {
  using C = Cfg<HD>;
  static constexpr int WAVES = WAVES_, NS = 2, SLOTS = SLOTS_;
  static constexpr int KCH = C::KROW / 8, VCH = C::VROW / 8;          // 16-byte chunks per K / V image row = KiB per image
  static constexpr int NPIECE = KCH + VCH;                            // 1-KiB DMA pieces per tile
  static constexpr int PW = (NPIECE + WAVES - 1) / WAVES;             // DMA instructions per wave and tile (a surplus one repeats the wave's previous piece)
  static constexpr int SLOT = NPIECE * 1024;
  static constexpr int RING = SLOTS * SLOT;
  static constexpr int TABS = WAVES * NS * 16 * G64_THLD * 4;
  static constexpr int LDS = RING + TABS + 16;                         // + the workgroup's "run the safe loop" flag
  static_assert(NPIECE > WAVES * (PW - 1) && PW >= 2, "every wave has a real piece to repeat");
  static_assert(RING >= WAVES * 16 * 80 * 4, "the prologue's per-wave scratch aliases the ring");
  static_assert(PW * (SLOTS - 2) <= 15 || SLOTS == 2, "vmcnt immediates used below");
};

// at most n tiles' DMA (PW instructions per wave and tile) may still be in flight
template <int PW>
__device__ __forceinline__ void g64_wait_tiles(int n) {
  switch (PW * n) {
#define S6D_G64_CASE(k) case k: S6D_VMCNT(k); break;
    S6D_G64_CASE(0) S6D_G64_CASE(3) S6D_G64_CASE(5) S6D_G64_CASE(6) S6D_G64_CASE(9) S6D_G64_CASE(10) S6D_G64_CASE(12)
#undef S6D_G64_CASE
    default: S6D_VMCNT(15); break;              // 15 or more (PW (SLOTS - 2) <= 15 is asserted)
  }
}

template <int HD, int WAVES, int SLOTS>
__global__ __launch_bounds__(WAVES * 64) void attn_global64_kernel(AttnParams p) {
  using C = Cfg<HD>;
  using G = G64<HD, WAVES, SLOTS>;
  constexpr int NS = G::NS, PW = G::PW;
  S6D_DYN_LDS(smem);
  float *tabs = reinterpret_cast<float *>(smem + G::RING);
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int g = lane >> 4, c = lane & 15;
  // workgroup -> (image, head, query tile): the query tiles of one (image, head) stay on ONE XCD (K / V re-reads hit its L2)
  const int nqt = p.T / (WAVES * 16 * NS);
  const int nbh = p.B * p.nh;
  int id = blockIdx.x, qt, bh;
  if ((nbh & 7) == 0) {
    const int xcd = id & 7, loc = id >> 3;
    qt = loc % nqt;
    bh = (loc / nqt) * 8 + xcd;
  } else {
    qt = id % nqt;
    bh = id / nqt;
  }
  const int head = bh % p.nh, b = bh / p.nh;
  StripState<HD, NS> st;
  int q0[NS];
  float *thm[NS];
#pragma unroll
  for (int n = 0; n < NS; ++n) {
    q0[n] = ((qt * WAVES + wave) * NS + n) * 16;
    load_q<HD>(p, b, 0, 0, head, q0[n], st.qf[n], lane);
    st.qy[n] = q0[n] >> 6;
    st.qx[n] = (q0[n] & 63) + c;
    st.m_run[n] = -1e30f;
    st.lacc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int dt = 0; dt < C::DT; ++dt) st.oacc[n][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    st.th[n] = nullptr;
    st.tw[n] = nullptr;
    // a strip's 16 queries share qy; tile t is key row ky = t:  th[c][t] = rel_h[qy - t + 63] . q_c, and
    // twr = rel_w[qx_c - kx + 63] . q_c gathered from G[c][jj] = rel_w[q0x + jj] . q_c (jj < 80; per-wave scratch in the ring)
    float *th = tabs + (size_t)(wave * NS + n) * 16 * G64_THLD;
    float *Gs = reinterpret_cast<float *>(smem) + (size_t)wave * 16 * 80;
    const int q0y = q0[n] >> 6, q0x = q0[n] & 63;
    build_table<HD, 4>(p.rel_h, q0y + 63, -1, st.qf[n], th, G64_THLD, lane);
    build_table<HD, 5>(p.rel_w, q0x, 1, st.qf[n], Gs, 80, lane);
    S6D_WAVE_RENDEZVOUS();   // (same-wave LDS order; on the GPU the wave's LDS operations execute in program order)
#pragma unroll
    for (int sub = 0; sub < 4; ++sub)
#pragma unroll
      for (int r = 0; r < 4; ++r) st.twr[n][sub * 4 + r] = Gs[c * 80 + (c + 63 - (sub * 16 + g * 4 + r))];
    S6D_WAVE_RENDEZVOUS();   // (the second strip's table overwrites the scratch)
    thm[n] = th;
  }
  // ---- this lane's DMA sources: piece q = wave + WAVES i of a tile is 64 consecutive chunks of the K image (q < KCH) or of the
  // V image; chunk -> (key row, part); zero-padded parts read a 16-byte zero; a wave without an i-th piece repeats its previous one
  // (same bytes to the same place), so that every wave has PW instructions per tile in flight and the waits count whole tiles
  const u16 *src[PW];
  long inc[PW];
  int dsto[PW];
  const long tstride = 64L * p.tok_stride;
#pragma unroll
  for (int i = 0; i < PW; ++i) {
    const int q = wave + WAVES * i < G::NPIECE ? wave + WAVES * i : wave + WAVES * (i - 1);
    const bool isk = q < G::KCH;
    const int piece = isk ? q : q - G::KCH, rowch = isk ? G::KCH : G::VCH;
    const int j = piece * 64 + lane;
    const int row = j / rowch, pp = j - row * rowch;
    const int part = isk ? (pp < C::KPARTS ? pp ^ kswz(row) : C::KPARTS) : pp;
    const bool data = part * 8 < HD;
    src[i] = data ? qkv_at(p, (size_t)b * p.T + row, isk ? 1 : 2, head) + part * 8 : reinterpret_cast<const u16 *>(&g_attn_zero16);
    inc[i] = data ? tstride : 0;
    dsto[i] = q * 1024;
  }
  auto issue = [&](int slot) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < PW; ++i) {
      S6D_LDS(char) *dst = (S6D_LDS(char) *)smem + slot * G::SLOT + dsto[i];
      lds_dma16_m0(src[i], dst);
      src[i] += inc[i];
    }
  };
  const int ntile = p.T / 64;
  constexpr int D = SLOTS - 1;                      // look-ahead in tiles
  static_assert(D >= 1 && D <= 6, "ring depth");
  // column bias as the score chain's C operand (process_tile_nomax): tw / scale_log2, four key columns per register quad
  f32x4 cbias[NS][4];
  {
    const float inv = 1.0f / p.scale_log2;
#pragma unroll
    for (int n = 0; n < NS; ++n)
#pragma unroll
      for (int sub = 0; sub < 4; ++sub)
#pragma unroll
        for (int r = 0; r < 4; ++r) cbias[n][sub][r] = st.twr[n][sub * 4 + r] * inv;
  }
  int *redo = reinterpret_cast<int *>(smem + G::RING + G::TABS);
  const u16 *src0[PW];
#pragma unroll
  for (int i = 0; i < PW; ++i) src0[i] = src[i];
  long long tk[6] = {0, 0, 0, 0, 0, 0}, tsum[5] = {0, 0, 0, 0, 0};
  int slot = 0;
  // everything of a tile in front of its arithmetic: this wave's pieces have landed, everybody's have (barrier; every wave is past
  // tile t - 1, so its slot is free), the DMA of tile t + D is issued into that slot, the row-bias words of the tile are read
  auto tile_head = [&](int t, float (&thv)[NS]) __attribute__((always_inline)) -> const u16 * {
    S6D_TICK(tk, 0);
    g64_wait_tiles<PW>(min(D - 1, ntile - 1 - t));
    S6D_LGKM0();
    __builtin_amdgcn_s_barrier();
    S6D_TICK(tk, 1);
    if (t + D < ntile && !(kAbl & 1)) issue(slot >= 1 ? slot - 1 : SLOTS - 1);
#pragma unroll
    for (int n = 0; n < NS; ++n) thv[n] = thm[n][c * G64_THLD + t];
    S6D_TICK(tk, 2);
    const u16 *Kl = reinterpret_cast<const u16 *>(smem + slot * G::SLOT);
    slot = slot == SLOTS - 1 ? 0 : slot + 1;
    return Kl;
  };
  auto prime = [&]() __attribute__((always_inline)) {
    __syncthreads();                                // every wave is done with its scratch (it aliases the ring) / with the first pass
    if (tid == 0) *redo = 0;
#pragma unroll
    for (int d = 0; d < D; ++d) issue(d);
    slot = 0;
  };
  // (The alternative was a static s_setprio 1 for the second-dispatched half of the workgroup over the whole tile loop: 0.9 % slower,
  // docs/NOTEBOOK_r5.md, profiles/r05_attn_nomax_variants.txt.)
  bool done = false;
  if (S6D_G64_NOMAX && !S6D_G64_TIMING) {
    // ---- pass A: tile 0 with the running-maximum arithmetic (it sets m_run), every later tile without a maximum ------------------
    prime();
    {
      float thv[NS];
      const u16 *Kl = tile_head(0, thv);
      process_tile<HD, 1, NS, true, kGlbPrio>(p, Kl, Kl + 64 * C::KROW, 0, st, thv, lane, tk);
    }
    for (int t = 1; t < ntile; ++t) {
      float thv[NS], nb[NS];
      const u16 *Kl = tile_head(t, thv);
#pragma unroll
      for (int n = 0; n < NS; ++n) nb[n] = thv[n] - st.m_run[n];
      process_tile_nomax<HD, NS, true>(p, Kl, Kl + 64 * C::KROW, st, cbias, nb, lane);
    }
    // a row sum that left the comfortable range (or is inf / NaN): the whole workgroup repeats its tiles with the running maximum
    bool bad = false;
#pragma unroll
    for (int n = 0; n < NS; ++n) {
      bad |= !(st.lacc[n][0] < kNoMaxSumLimit);
#pragma unroll
      for (int dt = 0; dt < C::DT; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) bad |= !(fabsf(st.oacc[n][dt][r]) < kNoMaxFinite);
    }
    if (__any(bad) && lane == 0) *redo = 1;
    __syncthreads();
    done = *redo == 0;
    if (!done) {
#pragma unroll
      for (int n = 0; n < NS; ++n) {
        st.m_run[n] = -1e30f;
        st.lacc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int dt = 0; dt < C::DT; ++dt) st.oacc[n][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int i = 0; i < PW; ++i) src[i] = src0[i];
    }
  }
  if (!done) {
    // ---- pass B: the round-4 kernel (every tile with the running maximum); the fallback of pass A ---------------------------------
    prime();
    for (int t = 0; t < ntile; ++t) {
      float thv[NS];
      const u16 *Kl = tile_head(t, thv);
      if (!(kAbl & 2)) process_tile<HD, 1, NS, true, kGlbPrio>(p, Kl, Kl + 64 * C::KROW, t * 64, st, thv, lane, tk);
      S6D_TICK(tk, 5);
      if (S6D_G64_TIMING)
#pragma unroll
        for (int i = 0; i < 5; ++i) tsum[i] += tk[i + 1] - tk[i];
    }
  }
#pragma unroll
  for (int n = 0; n < NS; ++n) store_strip<HD>(p, b, 0, 0, head, q0[n], st.lacc[n][0], st.oacc[n], lane);
  if (S6D_G64_TIMING && blockIdx.x == 8 && lane == 0) {             // the caller of a probe build leaves 4 KiB behind the output
    long long *dbg = reinterpret_cast<long long *>(p.out + (size_t)p.B * p.T * p.nh * HD);
#pragma unroll
    for (int i = 0; i < 5; ++i) dbg[wave * 5 + i] = tsum[i];
  }
}

template <int HD>
static int launch_global(AttnParams p, hipStream_t st) {
  using C = Cfg<HD>;
  const bool bias = p.rel_h != nullptr;
  if (p.T % 64 != 0) return S6D_EUNSUPPORTED;                  // global grids: 16x16, 32x32, 64x64 ...
  if (bias && p.S == 64) {
    using G = G64<HD, S6D_G64_WAVES, S6D_G64_SLOTS>;
    static_assert(G::LDS <= 160 * 1024, "ring + tables fit the CU's LDS");
    launch_lds(attn_global64_kernel<HD, G::WAVES, G::SLOTS>, (unsigned)(p.B * p.nh * (p.T / (G::WAVES * 32))), G::WAVES * 64, G::LDS, st, p);
    return launch_status();
  }
  // 4 waves: two workgroups per CU.  The alternative was 8 (S6D_GLB_WAVES: one workgroup, each staged tile shared by twice the
  // queries): 1.78 against 1.89 ms, behind attn_global64_kernel's 1.73 (docs/NOTEBOOK_r1_r4.md section 4.2, profiles/r02_attn_variants.txt)
  constexpr int WAVES = 4, NS = 2;
  const size_t ring = (size_t)2 * 64 * (C::KROW + C::VROW) * 2;
  const int nqt = (p.T + WAVES * 16 * NS - 1) / (WAVES * 16 * NS);
  const unsigned grid = (unsigned)(p.B * p.nh * nqt);
  const size_t lds = bias ? ring + (size_t)WAVES * NS * 2 * 16 * p.LT * 4 : ring;
  if (lds > 160 * 1024) return S6D_EUNSUPPORTED;
  if (bias) {
    launch_lds(attn_global_kernel<HD, WAVES, 0>, grid, WAVES * 64, lds, st, p);
  } else {
    launch_lds(attn_global_kernel<HD, WAVES, 2>, grid, WAVES * 64, lds, st, p);
  }
  return launch_status();
}

}  // namespace S6D_ATTN_NS
