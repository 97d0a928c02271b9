// All-resident attention: one workgroup per (image, window, head) with every key slot in LDS.  With the decomposed position bias it
// serves windows the row-padded kernels do not take (s6d_attn_win16.h); without it, it is the SEQUENCE attention of DINOv2 (257
// tokens, bf16) and of the PEM's ViT-B (197 tokens, IEEE half): the two s6d_seq_attention entry points below, whose exported names
// follow the element type, so csrc/s6d_attn.hip and csrc/s6d_attn_f16.hip define them from this one text.
#pragma once
#include "s6d_attn_common.h"

namespace S6D_ATTN_NS {

__host__ __device__ inline int win_seq_krows(int T) { return (T + 15) & ~15; }
__host__ __device__ inline int win_seq_vrows(int T) { return (T + 31) & ~31; }
// tile `t` of a sequence against one strip: a full tile, or the tail with the 16-key sub-tiles that exist
template <int HD>
__device__ __forceinline__ void win_seq_tile(const AttnParams &p, const u16 *Kl, const u16 *Vl, int t, int nfull, int tail_subs,
                                             StripState<HD, 1> &st, int lane) {
  using C = Cfg<HD>;
  const float thv[1] = {0.f};
  const u16 *Kt = Kl + (size_t)t * 64 * C::KROW, *Vt = Vl + (size_t)t * 64 * C::VROW;
  if (t < nfull) {
    process_tile<HD, 2, 1>(p, Kt, Vt, t * 64, st, thv, lane);
    return;
  }
  switch (tail_subs) {                                              // wave-uniform
    case 1: process_tile<HD, 2, 1, false, false, 1>(p, Kt, Vt, t * 64, st, thv, lane); break;
    case 2: process_tile<HD, 2, 1, false, false, 2>(p, Kt, Vt, t * 64, st, thv, lane); break;
    case 3: process_tile<HD, 2, 1, false, false, 3>(p, Kt, Vt, t * 64, st, thv, lane); break;
    default: process_tile<HD, 2, 1, false, false, 4>(p, Kt, Vt, t * 64, st, thv, lane); break;
  }
}

// ---- windowed: one workgroup per (image, window, head); every key slot LDS resident ------------------------
template <int HD, int WAVES, bool BIAS>
__global__ __launch_bounds__(WAVES * 64) void attn_window_kernel(AttnParams p) {
  using C = Cfg<HD>;
  constexpr int MODE = BIAS ? 0 : 2;
  S6D_DYN_LDS(smem);
  const int ntile = (p.T + 63) / 64;
  // no bias (sequences): COMPACT images -- K rows up to the last 16-key sub-tile that exists, V rows up to the last 32-key step
  // (win_seq_tile above skips the absent sub-tiles of the tail tile).  257 tokens x head dim 64: 272 x 144 + 288 x 144 = 78.75 KiB instead
  // of 320 rows of both = 95 KiB, i.e. two workgroups per CU: one fetches its item while the other computes (round 4).
  const int krows = BIAS ? ntile * 64 : win_seq_krows(p.T), vrows = BIAS ? ntile * 64 : win_seq_vrows(p.T);
  u16 *Kl = reinterpret_cast<u16 *>(smem);                         // [krows][KROW]
  u16 *Vl = Kl + (size_t)krows * C::KROW;                          // [vrows][VROW]
  float *tabs = reinterpret_cast<float *>(Vl + (size_t)vrows * C::VROW);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  float *th = tabs + (size_t)wave * 2 * 16 * p.LT, *tw = th + 16 * p.LT;

  WinItem item;
  item.decode(p, blockIdx.x);
  const int head = item.head, wx = item.wx, wy = item.wy, b = item.b;
  {
    // the loads of up to SB tiles are issued before the first of them is stored: one exposed fetch latency per SB tiles instead of
    // one per tile (T = 257 / 197 keys = 5 / 4 tiles: the whole item in one batch)
    constexpr int SB = 5;
    Stager<HD, WAVES * 64> st[SB];
    for (int t0 = 0; t0 < ntile; t0 += SB) {
#pragma unroll
      for (int i = 0; i < SB; ++i)
        if (t0 + i < ntile) st[i].load(p, b, wy, wx, head, (t0 + i) * 64, tid);
#pragma unroll
      for (int i = 0; i < SB; ++i)
        if (t0 + i < ntile)
          st[i].store(Kl + (size_t)(t0 + i) * 64 * C::KROW, Vl + (size_t)(t0 + i) * 64 * C::VROW, tid, krows - (t0 + i) * 64,
                      vrows - (t0 + i) * 64);
    }
  }
  __syncthreads();

  const int nstrip = (p.T + 15) / 16;
  for (int strip = wave; strip < nstrip; strip += WAVES) {
    const int q0 = strip * 16;
    StripState<HD, 1> st;
    load_q<HD>(p, b, wy, wx, head, q0, st.qf[0], lane);
    st.th[0] = th; st.tw[0] = tw;
    if (BIAS) {
      for (int jt = 0; jt < p.LT / 16; ++jt) {
        build_table<HD, 1>(p.rel_h, jt * 16, 1, st.qf[0], th + jt * 16, p.LT, lane);
        build_table<HD, 1>(p.rel_w, jt * 16, 1, st.qf[0], tw + jt * 16, p.LT, lane);
      }
    }
    const int qi = min(q0 + (lane & 15), p.T - 1);
    st.qy[0] = div_S(p, qi); st.qx[0] = qi - st.qy[0] * p.S;
    st.m_run[0] = -1e30f; st.lacc[0] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 16; ++i) st.twr[0][i] = 0.f;
#pragma unroll
    for (int dt = 0; dt < C::DT; ++dt) st.oacc[0][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float thv[1] = {0.f};
    if (BIAS) {
      for (int t = 0; t < ntile; ++t)
        process_tile<HD, MODE, 1>(p, Kl + (size_t)t * 64 * C::KROW, Vl + (size_t)t * 64 * C::VROW, t * 64, st, thv, lane);
    } else {
      const int nfull = p.T >> 6, tail_subs = ((p.T & 63) + 15) >> 4;
      for (int t = 0; t < ntile; ++t) win_seq_tile<HD>(p, Kl, Vl, t, nfull, tail_subs, st, lane);
    }
    store_strip<HD>(p, b, wy, wx, head, q0, st.lacc[0][0], st.oacc[0], lane);
  }
}

// WITH_BIAS = false leaves attn_window_kernel<., ., true> out of the unit (the sequence entry points never carry a position bias; the
// half unit builds nothing else).
template <int HD, bool WITH_BIAS>
static int launch_window(AttnParams p, hipStream_t st) {
  using C = Cfg<HD>;
  constexpr int WAVES = 8;
  const bool bias = p.rel_h != nullptr;
  if (bias && !WITH_BIAS) return S6D_EUNSUPPORTED;               // a kernel this unit does not hold is an error, not a fall-back
  const int ntile = (p.T + 63) / 64;
  const size_t lds = bias ? (size_t)ntile * 64 * (C::KROW + C::VROW) * 2 + (size_t)WAVES * 2 * 16 * p.LT * 4
                          : ((size_t)win_seq_krows(p.T) * C::KROW + (size_t)win_seq_vrows(p.T) * C::VROW) * 2;
  if (lds > 160 * 1024) return S6D_EUNSUPPORTED;
  const unsigned grid = (unsigned)(p.B * p.nwy * p.nwx * p.nh);
  if (!bias) {
    launch_lds(attn_window_kernel<HD, WAVES, false>, grid, WAVES * 64, lds, st, p);
  } else if constexpr (WITH_BIAS) {
    launch_lds(attn_window_kernel<HD, WAVES, true>, grid, WAVES * 64, lds, st, p);
  }
  return launch_status();
}

}  // namespace S6D_ATTN_NS

#if S6D_ATTN_F16
#define S6D_SEQ_ATTENTION s6d_seq_attention_f16
#define S6D_SEQ_ATTENTION_STRIDED s6d_seq_attention_strided_f16
#else
#define S6D_SEQ_ATTENTION s6d_seq_attention_bf16
#define S6D_SEQ_ATTENTION_STRIDED s6d_seq_attention_strided_bf16
#endif
// q / k / v element (sequence b, token n, which, head h, d) sits at qkv + (b N + n) tok_stride + which which_stride + h head_stride + d:
//   token-major (the raw Linear output (B, N, 3, nh, hd)):  tok_stride = 3 nh hd, which_stride = nh hd, head_stride = hd
//   head-major  ((3, nh, B N, hd), the qkv GEMM's column-block epilogue):  tok_stride = hd, head_stride = B N hd, which_stride = nh B N hd
// Head-major makes the K / V rows of one (sequence, head) ONE contiguous run (257 x 128 B = 32 KB) instead of 257 pieces of 128 B
// strided by 6 KB: measured on the DINOv2 shape, the fetch of the token-major pieces ALONE costs 136 us per launch (2.3 TB/s).
extern "C" int S6D_SEQ_ATTENTION_STRIDED(const void *qkv, long tok_stride, long which_stride, long head_stride, int B, int N,
                                         int num_heads, int head_dim, float scale, void *out, void *stream) {
  using namespace S6D_ATTN_NS;
  if (B < 0 || N <= 0 || num_heads <= 0 || head_dim <= 0) return S6D_EINVAL;
  if (tok_stride < head_dim || (tok_stride % 8) || (which_stride % 8) || (head_stride % 8)) return S6D_EINVAL;   // 16-byte chunks
  if (B == 0) return S6D_OK;
  if (!qkv || !out || ((uintptr_t)qkv & 15)) return S6D_EINVAL;
  // a 1 x N "image" attended as ONE all-resident window of N key slots, no positional bias
  AttnParams p;
  p.qkv = (const u16 *)qkv; p.qkv_bias = nullptr;                 // slots past N read their sequence's first token (token_offset)
  p.rel_h = nullptr; p.rel_w = nullptr; p.out = (u16 *)out;
  p.B = B; p.H = 1; p.W = N; p.nh = num_heads; p.ws = N;
  p.S = N; p.T = N; p.nwx = 1; p.nwy = 1; p.LT = 16;
  p.magicS = (unsigned)(((1ull << 32) + (unsigned)N - 1) / (unsigned)N);
  p.scale_log2 = scale * kLog2e;
  p.tok_stride = tok_stride; p.which_stride = which_stride; p.head_stride = head_stride;
  hipStream_t st = as_stream(stream);
  switch (head_dim) {
    case 80: return launch_window<80, false>(p, st);
    case 64: return launch_window<64, false>(p, st);
    default: return S6D_EUNSUPPORTED;
  }
}

extern "C" int S6D_SEQ_ATTENTION(const void *qkv, int B, int N, int num_heads, int head_dim, float scale, void *out,
                                 void *stream) {
  if (num_heads <= 0 || head_dim <= 0) return S6D_EINVAL;
  return S6D_SEQ_ATTENTION_STRIDED(qkv, 3L * num_heads * head_dim, (long)num_heads * head_dim, head_dim, B, N, num_heads, head_dim,
                                   scale, out, stream);
}
