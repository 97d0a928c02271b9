// Fused ViT attention, bf16 unit: every kernel family (csrc/s6d_attn_common.h has the overview and the MFMA mapping), the dispatch
// between them and the s6d_win_attention_* entry points of the SAM image encoder; s6d_seq_attention_bf16 / _strided_bf16 come from
// csrc/s6d_attn_seq.h.  csrc/s6d_attn_f16.hip is the IEEE-half unit (sequences only).
#include "s6d_attn_common.h"
#include "s6d_attn_seq.h"
#include "s6d_attn_win16.h"
#include "s6d_attn_global.h"

#if !S6D_ATTN_F16   // bf16 only: the half unit (csrc/s6d_attn_f16.hip) has no dispatch and no s6d_win_attention_* entry points
namespace S6D_ATTN_NS {

// rel (L,HD) -> padded (rows,HDP), zero filled
__global__ void pad_rel_kernel(const u16 *__restrict__ rel_h, const u16 *__restrict__ rel_w, int L, int HD, int HDP,
                               int rows, u16 *__restrict__ out) {
  const int n = rows * HDP;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < 2 * n; i += gridDim.x * blockDim.x) {
    const int which = i >= n, ii = which ? i - n : i;
    const int j = ii / HDP, d = ii - j * HDP;
    const u16 *src = which ? rel_w : rel_h;
    out[i] = (j < L && d < HD) ? src[j * HD + d] : (u16)0;
  }
}

// row-padded windows (S <= 16, with bias) | all-resident windows | global attention over the H x W grid
template <int HD>
static int launch_attn(AttnParams p, hipStream_t st) {
  if (p.ws > 0 && p.rel_h != nullptr && p.S <= 16) return launch_win16<HD>(p, st);
  if (p.ws > 0) return launch_window<HD, true>(p, st);
  return launch_global<HD>(p, st);
}

}  // namespace S6D_ATTN_NS

using namespace S6D_ATTN_NS;

extern "C" long s6d_win_attention_scratch_bytes(int H, int window, int head_dim) {
  const int S = window ? window : H;
  const int LT = ((2 * S - 1) + 15) / 16 * 16, HDP = (head_dim + 31) / 32 * 32;
  return 2L * (LT + 16) * HDP * 2;
}

// prepadded != 0: rel_scratch already holds the padded tables (s6d_win_attention_pad_rel_bf16, made once per weight version: the
// padding is a function of the two weight tables only and ran as a 5-us launch in front of every one of the 64 attention launches
// of a step); rel_h / rel_w are then only tested for presence.
static int win_attention_impl(const void *qkv, int head_major, const void *qkv_bias, const void *rel_h, const void *rel_w,
                              int B, int H, int W, int num_heads, int head_dim, int window, float scale,
                              void *rel_scratch, int prepadded, void *out, void *stream) {
  if (B < 0 || H <= 0 || W <= 0 || num_heads <= 0 || window < 0) return S6D_EINVAL;
  if (B == 0) return S6D_OK;
  if (!qkv || !qkv_bias || !out || ((rel_h == nullptr) != (rel_w == nullptr))) return S6D_EINVAL;
  if (window == 0 && H != W) return S6D_EUNSUPPORTED;
  if (window == 0 && (H * W) % 64 != 0) window = H;   // small odd grids: one all-resident "window" = whole grid
  AttnParams p;
  p.qkv = (const u16 *)qkv; p.qkv_bias = (const u16 *)qkv_bias;
  p.rel_h = (const u16 *)rel_h; p.rel_w = (const u16 *)rel_w; p.out = (u16 *)out;
  p.B = B; p.H = H; p.W = W; p.nh = num_heads; p.ws = window;
  p.S = window ? window : H; p.T = p.S * p.S;
  p.nwx = window ? (W + window - 1) / window : 1;
  p.nwy = window ? (H + window - 1) / window : 1;
  p.LT = ((2 * p.S - 1) + 15) / 16 * 16;
  p.magicS = (unsigned)(((1ull << 32) + (unsigned)p.S - 1) / (unsigned)p.S);
  p.scale_log2 = scale * kLog2e;
  if (head_major) {                              // (3, nh, B H W, hd): the qkv GEMM's column-block output
    const long plane = (long)B * H * W * head_dim;
    p.tok_stride = head_dim; p.head_stride = plane; p.which_stride = (long)num_heads * plane;
  } else {                                       // (B, H, W, 3, nh, hd): the raw Linear output
    p.tok_stride = 3L * num_heads * head_dim; p.which_stride = (long)num_heads * head_dim; p.head_stride = head_dim;
  }
  hipStream_t st = as_stream(stream);
  if (rel_h) {                                   // zero-padded table copies: unconditional loads in the kernels
    if (!rel_scratch) return S6D_EINVAL;
    const int HDP = (head_dim + 31) / 32 * 32, rows = p.LT + 16;
    if (!prepadded)
      hipLaunchKernelGGL(pad_rel_kernel, dim3(16), dim3(256), 0, st, p.rel_h, p.rel_w, 2 * p.S - 1, head_dim, HDP, rows,
                         (u16 *)rel_scratch);
    p.rel_h = (const u16 *)rel_scratch;
    p.rel_w = p.rel_h + (size_t)rows * HDP;
  }
  switch (head_dim) {
    case 80: return launch_attn<80>(p, st);
    case 64: return launch_attn<64>(p, st);
    default: return S6D_EUNSUPPORTED;
  }
}

extern "C" int s6d_win_attention_layout_bf16(const void *qkv, int head_major, const void *qkv_bias, const void *rel_h, const void *rel_w,
                                             int B, int H, int W, int num_heads, int head_dim, int window, float scale,
                                             void *rel_scratch, void *out, void *stream) {
  return win_attention_impl(qkv, head_major, qkv_bias, rel_h, rel_w, B, H, W, num_heads, head_dim, window, scale, rel_scratch, 0, out, stream);
}

extern "C" int s6d_win_attention_bf16(const void *qkv, const void *qkv_bias, const void *rel_h, const void *rel_w,
                                      int B, int H, int W, int num_heads, int head_dim, int window, float scale,
                                      void *rel_scratch, void *out, void *stream) {
  return s6d_win_attention_layout_bf16(qkv, 0, qkv_bias, rel_h, rel_w, B, H, W, num_heads, head_dim, window, scale, rel_scratch, out,
                                       stream);
}

extern "C" int s6d_win_attention_pad_rel_bf16(const void *rel_h, const void *rel_w, int H, int window, int head_dim, void *rel_padded,
                                              void *stream) {
  if (!rel_h || !rel_w || !rel_padded || H <= 0 || window < 0 || head_dim <= 0) return S6D_EINVAL;
  const int S = window ? window : H, LT = ((2 * S - 1) + 15) / 16 * 16;
  const int HDP = (head_dim + 31) / 32 * 32, rows = LT + 16;
  hipLaunchKernelGGL(pad_rel_kernel, dim3(16), dim3(256), 0, as_stream(stream), (const u16 *)rel_h, (const u16 *)rel_w, 2 * S - 1, head_dim,
                     HDP, rows, (u16 *)rel_padded);
  return launch_status();
}

extern "C" int s6d_win_attention_prepadded_bf16(const void *qkv, int head_major, const void *qkv_bias, const void *rel_padded, int B, int H,
                                                int W, int num_heads, int head_dim, int window, float scale, void *out, void *stream) {
  if (!rel_padded) return S6D_EINVAL;
  return win_attention_impl(qkv, head_major, qkv_bias, rel_padded, rel_padded, B, H, W, num_heads, head_dim, window, scale,
                            const_cast<void *>(rel_padded), 1, out, stream);
}
#endif  // !S6D_ATTN_F16
