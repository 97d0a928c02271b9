// Run-length masks on the device (gfx950): dense masks -> runs, runs -> bit-packed masks, runs -> dense masks.  The format is DEFINED
// in include/sam6d_hip.h (s6d_rle_*) and DESIGN section 14; tests/rle_ref.py restates it in plain loops and every comparison is `equal`.
//
// Pixel order of the runs is COLUMN-major, p = x H + y; the runs of a mask alternate zeros, ones, ... beginning with zeros.  Dense
// masks and the packed words (those of s6d_mask_pack_u8) are ROW-major.  Every kernel therefore works on a BAND of columns whose
// pixels it keeps in LDS as column-major bits: column c of the band is `pitch` 64-bit words, bit y & 63 of word y >> 6 is row y.
// pitch = ceil(H / 64) | 1: odd, so that the 64 lanes of a wave, one column each, read 64 different 8-byte bank pairs also when
// ceil(H / 64) is a power of two.  A band holds at most `cap` words (S6D_RLE_BAND_WORDS, or s6d_set_rle_band_words for the tests).
//
// rle_encode_kernel<WRITE>  one workgroup per (mask, band of at most 64 columns).  Load: a wave takes 64 rows at a time, lane l reads
//                           the byte of column x0 + l in each of them (64 consecutive bytes per wave instruction) and ORs its bit
//                           into ONE register: after 64 rows the lane holds the word of its column -- the transposition costs
//                           nothing.  Transitions of word (c, w): T = bits ^ (bits << 1 | carry), carry = the pixel before the
//                           word's first (the top bit of the word above; at w = 0 the last pixel of column c - 1, for the band's first
//                           column read from the mask; 0 before pixel 0), the bits past H masked off.  Items are taken in
//                           (column, word) = position order, 256 at a time, with a workgroup exclusive scan of their popcounts.
//                           !WRITE: the band's transition count -> workspace[n, band].  WRITE: the same bits again; the band's first
//                           rank is the sum of the earlier bands' counts, and transition number r of the mask (0-based) stores
//                           its position in edges[offsets[n] + r].
// rle_runs_kernel           run_counts[n] = 1 + the mask's transitions (K transitions bound K + 1 runs: an all-zero mask is [H W],
//                           a mask whose pixel 0 is set has its first transition at 0 and so the leading zero run of length 0).
// rle_diff_kernel           one lane per run j of the whole batch: its mask by binary search in offsets, then
//                           counts[j] = e[i + 1] - e[i] with e = 0, the mask's transitions, H W.
// rle_check_kernel          one workgroup per mask: a negative count, an empty list, or a total != H W (from `ends`, the inclusive
//                           scan of all counts, minus the mask's base) sets status[1 + n] and lowers status[0] to n (atomicMin);
//                           area[n] = 0.  The decoders leave a refused mask alone: with monotone ends every loop below is bounded.
// rle_decode_kernel<DENSE>  one workgroup per (mask, band).  The band's first run by binary search in ends; lane i takes run
//                           first + i, + 256, ...: a one-run is clipped to the band and ORed into the LDS bits column by column --
//                           whole words by plain stores (no other run touches them), edge words by LDS atomicOr.  Then
//                           packed: a wave per (row, word of that row's band segment), lane k = pixel 64 j + k, the bit read from
//                             LDS, one __ballot; a word that lies wholly in the band's segment is stored, one shared with another
//                             band or row is ORed into the zeroed output (integer OR: no order dependence).  With one band the words
//                             are simply walked in order.  Popcounts -> one integer atomicAdd per wave into area[n].
//                           dense: a wave per row, lanes over the band's columns, bytes 0 / 1.
// Everything is integer work; the atomics are integer add / or / min: no result depends on N, on neighbours or on scheduling.
#include "s6d_common.h"

namespace s6d {

typedef unsigned long long u64;

constexpr int RLE_THREADS = 256;
constexpr int RLE_WAVES = RLE_THREADS / kWave;
constexpr int RLE_LDS_WORDS = S6D_RLE_BAND_WORDS;
constexpr int RLE_OK_MASK = 0x7fffffff;                                  // status[0] while no mask is refused

int g_s6d_rle_band_words = 0;                                            // s6d_set_rle_band_words; 0 = RLE_LDS_WORDS

struct RlePlan {
  int nw, pitch;                                                         // words of a column; LDS words between columns
  int bc, bands, row_words;                                              // decoders: columns of a band, bands, words a row segment can touch
  int ec, ebands;                                                        // encoder: columns of a band (<= 64), bands
  long HW, words;
};

static int rle_plan(int N, int H, int W, RlePlan *pl) {
  if (N < 0 || H < 1 || W < 1) return S6D_EINVAL;
  const long HW = (long)H * W;
  if (HW > 0x7fffffffL) return S6D_EINVAL;
  const int cap = g_s6d_rle_band_words > 0 ? g_s6d_rle_band_words : RLE_LDS_WORDS;
  const int nw = (H + 63) / 64, pitch = nw | 1;
  if (pitch > cap) return S6D_EUNSUPPORTED;                              // (one column does not fit: H > 64 cap)
  int bc = cap / pitch;
  if (bc >= 64) bc &= ~63;                                               // whole words per row segment when W is a multiple of 64
  if (bc > W) bc = W;
  int ec = cap / pitch;
  if (ec > 64) ec = 64;
  if (ec > W) ec = W;
  const long bands = (W + bc - 1) / bc, ebands = (W + ec - 1) / ec;
  if (N * bands > 0x7fffffffL || N * ebands > 0x7fffffffL) return S6D_EUNSUPPORTED;
  pl->nw = nw;
  pl->pitch = pitch;
  pl->bc = bc;
  pl->bands = (int)bands;
  pl->row_words = (bc + 62) / 64 + 1;
  pl->ec = ec;
  pl->ebands = (int)ebands;
  pl->HW = HW;
  pl->words = (HW + 63) / 64;
  return S6D_OK;
}

// inclusive sum over the lanes 0 .. lane of the wave
__device__ __forceinline__ int wave_inclusive_sum(int v) {
  const int lane = lane_id();
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int t = __shfl(v, lane >= o ? lane - o : lane);
    if (lane >= o) v += t;
  }
  return v;
}

template <bool WRITE>
__global__ __launch_bounds__(RLE_THREADS) void rle_encode_kernel(const uint8_t *__restrict__ masks, int H, int W, int nw, int pitch,
                                                                 int ec, int ebands, int *band_counts,
                                                                 const long *__restrict__ offsets, long R, int *__restrict__ edges) {
  __shared__ u64 B[RLE_LDS_WORDS];
  __shared__ int wsum[RLE_WAVES];
  const int n = blockIdx.x / ebands, b = blockIdx.x - n * ebands;
  const int x0 = b * ec, ncols = min(ec, W - x0);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint8_t *M = masks + (size_t)n * H * W;
  for (int rc = wave; rc < nw; rc += RLE_WAVES) {
    if (lane >= ncols) continue;
    const int y0 = rc * 64, rows = min(64, H - y0);
    const uint8_t *src = M + (size_t)y0 * W + x0 + lane;
    u64 word = 0;
#pragma unroll 8
    for (int r = 0; r < rows; ++r) word |= (u64)(src[(size_t)r * W] != 0) << r;
    B[lane * pitch + rc] = word;
  }
  const int before = x0 > 0 ? (M[(size_t)(H - 1) * W + x0 - 1] != 0) : 0;  // the pixel before the band's first
  int rank = 0;                                                          // WRITE: the rank of the band's first transition in the mask
  long lo = 0, hi = 0;
  if (WRITE) {
    lo = offsets[n];
    hi = offsets[n + 1];
    if (lo < 0 || hi > R || hi < lo) return;                             // (the whole workgroup: offsets that do not fit the arrays)
    int s = 0;
    for (int k = threadIdx.x; k < b; k += RLE_THREADS) s += band_counts[(size_t)n * ebands + k];
    s = wave_sum_i32(s);
    if (lane == 0) wsum[wave] = s;
    __syncthreads();
    for (int k = 0; k < RLE_WAVES; ++k) rank += wsum[k];
  }
  __syncthreads();                                                       // the bits are in LDS; wsum is free again
  const int items = ncols * nw;
  for (int i0 = 0; i0 < items; i0 += RLE_THREADS) {
    const int i = i0 + threadIdx.x;
    u64 T = 0;
    int pos0 = 0;
    if (i < items) {
      const int c = i / nw, w = i - c * nw;
      const u64 bits = B[c * pitch + w];
      u64 carry = before;
      if (w > 0) carry = B[c * pitch + w - 1] >> 63;
      else if (c > 0) carry = (B[(c - 1) * pitch + ((H - 1) >> 6)] >> ((H - 1) & 63)) & 1ull;
      T = bits ^ ((bits << 1) | carry);
      const int nb = H - 64 * w;
      if (nb < 64) T &= (1ull << nb) - 1ull;
      pos0 = (x0 + c) * H + 64 * w;
    }
    const int cnt = __popcll(T);
    const int incl = wave_inclusive_sum(cnt);
    if (lane == kWave - 1) wsum[wave] = incl;
    __syncthreads();
    int off = 0, tot = 0;
    for (int k = 0; k < RLE_WAVES; ++k) {
      if (k < wave) off += wsum[k];
      tot += wsum[k];
    }
    __syncthreads();                                                     // everyone has read wsum before the next round's stores
    if (WRITE) {
      long slot = lo + rank + off + incl - cnt;
      while (T != 0) {
        const int k = __ffsll(T) - 1;
        T &= T - 1ull;
        if (slot < hi) edges[slot] = pos0 + k;
        ++slot;
      }
    }
    rank += tot;
  }
  if (!WRITE && threadIdx.x == 0) band_counts[blockIdx.x] = rank;
}

__global__ __launch_bounds__(RLE_THREADS) void rle_runs_kernel(const int *__restrict__ band_counts, int N, int ebands,
                                                               int *__restrict__ run_counts) {
  const int n = blockIdx.x * RLE_THREADS + threadIdx.x;
  if (n >= N) return;
  int s = 1;
  for (int k = 0; k < ebands; ++k) s += band_counts[(size_t)n * ebands + k];
  run_counts[n] = s;
}

__global__ __launch_bounds__(RLE_THREADS) void rle_diff_kernel(const long *__restrict__ offsets, int N, long R, int HW,
                                                               const int *__restrict__ edges, int *__restrict__ counts) {
  const long j = (long)blockIdx.x * RLE_THREADS + threadIdx.x;
  if (j >= R) return;
  int a = 0, z = N - 1;                                                  // the last mask whose list begins at or before j
  while (a < z) {
    const int m = (a + z + 1) >> 1;
    if (offsets[m] <= j) a = m;
    else z = m - 1;
  }
  const long lo = offsets[a], hi = offsets[a + 1];
  if (j < lo || j >= hi) return;
  const int e0 = j > lo ? edges[j - 1] : 0, e1 = j + 1 < hi ? edges[j] : HW;
  counts[j] = e1 - e0;
}

__global__ void rle_status_init_kernel(int *status) { status[0] = RLE_OK_MASK; }

__global__ __launch_bounds__(RLE_THREADS) void rle_check_kernel(const int *__restrict__ counts, const long *__restrict__ offsets,
                                                                const long *__restrict__ ends, long R, long HW, int *__restrict__ area,
                                                                int *status) {
  __shared__ int negative;
  const int n = blockIdx.x;
  const long lo = offsets[n], hi = offsets[n + 1];
  bool bad = lo < 0 || hi > R || hi <= lo;                               // (an empty list has no zero run)
  if (threadIdx.x == 0) negative = 0;
  __syncthreads();
  if (!bad) {
    bool neg = false;
    for (long i = lo + threadIdx.x; i < hi; i += RLE_THREADS) neg = neg || counts[i] < 0;
    if (neg) negative = 1;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (!bad) bad = negative != 0 || ends[hi - 1] - (lo > 0 ? ends[lo - 1] : 0L) != HW;
  status[1 + n] = bad ? 1 : 0;
  if (bad) atomicMin(&status[0], n);
  if (area != nullptr) area[n] = 0;
}

// the bits [y, y + len) of one LDS column
__device__ __forceinline__ void rle_set_bits(u64 *col, int y, int len) {
  const int last = y + len - 1, w0 = y >> 6, w1 = last >> 6;
  for (int w = w0; w <= w1; ++w) {
    u64 m = ~0ull;
    if (w == w0) m &= ~0ull << (y & 63);
    if (w == w1) m &= ~0ull >> (63 - (last & 63));
    if (m == ~0ull) col[w] = m;
    else atomicOr(&col[w], m);
  }
}

template <bool DENSE>
__global__ __launch_bounds__(RLE_THREADS) void rle_decode_kernel(const long *__restrict__ offsets, const long *__restrict__ ends, int H,
                                                                 int W, int pitch, int bc, int bands, int row_words, long words,
                                                                 const int *__restrict__ status, u64 *packed, int *area,
                                                                 uint8_t *__restrict__ dense) {
  __shared__ u64 B[RLE_LDS_WORDS];
  const int n = blockIdx.x / bands, b = blockIdx.x - n * bands;
  if (status[1 + n] != 0) return;                                        // (the whole workgroup) a refused mask
  const int x0 = b * bc, x1 = min(W, x0 + bc), ncols = x1 - x0;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int i = threadIdx.x; i < ncols * pitch; i += RLE_THREADS) B[i] = 0ull;
  __syncthreads();
  const long lo = offsets[n], hi = offsets[n + 1], base = lo > 0 ? ends[lo - 1] : 0L;
  const long p0 = (long)x0 * H, p1 = (long)x1 * H;
  long first = lo, z = hi;                                               // the first run that ends after p0
  while (first < z) {
    const long m = (first + z) >> 1;
    if (ends[m] - base > p0) z = m;
    else first = m + 1;
  }
  for (long i = first + threadIdx.x; i < hi; i += RLE_THREADS) {
    long s = i > lo ? ends[i - 1] - base : 0L, e = ends[i] - base;
    if (s >= p1) break;
    if (((i - lo) & 1L) == 0) continue;                                  // a run of zeros
    s = s > p0 ? s : p0;
    e = e < p1 ? e : p1;
    int len = (int)(e - s);
    if (len <= 0) continue;
    const int q = (int)(s - p0);                                         // < ncols H <= 64 cap
    int c = q / H, y = q - c * H;
    while (len > 0) {
      const int seg = min(len, H - y);
      rle_set_bits(B + c * pitch, y, seg);
      len -= seg;
      y = 0;
      ++c;
    }
  }
  __syncthreads();
  if (DENSE) {
    uint8_t *D = dense + (size_t)n * H * W;
    for (int y = wave; y < H; y += RLE_WAVES)
      for (int c = lane; c < ncols; c += kWave) D[(size_t)y * W + x0 + c] = (uint8_t)((B[c * pitch + (y >> 6)] >> (y & 63)) & 1ull);
    return;
  }
  u64 *P = packed + (size_t)n * words;
  const long HW = (long)H * W;
  int cnt = 0;
  if (bands == 1) {
    for (long j = wave; j < words; j += RLE_WAVES) {
      const long p = 64 * j + lane;
      bool bit = false;
      if (p < HW) {
        const int y = (int)p / W, x = (int)p - y * W;
        bit = ((B[x * pitch + (y >> 6)] >> (y & 63)) & 1ull) != 0;
      }
      const u64 v = __ballot(bit);
      cnt += __popcll(v);
      if (lane == 0) P[j] = v;
    }
  } else {
    const int tasks = H * row_words;
    for (int t = wave; t < tasks; t += RLE_WAVES) {
      const int y = t / row_words, k = t - y * row_words;
      const long r0 = (long)y * W + x0, r1 = (long)y * W + x1;           // the band's pixels of row y, row-major
      const long j = (r0 >> 6) + k;
      if (j > ((r1 - 1) >> 6)) continue;                                 // (the whole wave)
      const long p = 64 * j + lane;
      const bool bit = p >= r0 && p < r1 && ((B[(int)(p - r0) * pitch + (y >> 6)] >> (y & 63)) & 1ull) != 0;
      const u64 v = __ballot(bit);
      cnt += __popcll(v);
      const long wend = 64 * j + 64 < HW ? 64 * j + 64 : HW;
      if (lane == 0) {
        if (64 * j >= r0 && wend <= r1) P[j] = v;                        // the word has no pixel outside this row segment
        else if (v != 0) atomicOr(&P[j], v);
      }
    }
  }
  if (lane == 0 && cnt != 0) atomicAdd(&area[n], cnt);
}

// true when every packed word lies inside one (row, band) segment: nothing is ORed, the output needs no zeroing
static bool rle_words_owned(const RlePlan &pl, int W) { return pl.bands == 1 || (W % 64 == 0 && pl.bc % 64 == 0); }

template <bool DENSE>
static int rle_decode(const int32_t *counts, const long *offsets, const long *ends, int N, long R, int H, int W, int32_t *status,
                      uint64_t *packed, int32_t *area, uint8_t *dense, void *stream) {
  RlePlan pl;
  const int rc = rle_plan(N, H, W, &pl);
  if (rc != S6D_OK) return rc;
  if (R < N) return S6D_EINVAL;                                          // (every list has at least its zero run)
  if (N == 0) return S6D_OK;
  if (!counts || !offsets || !ends || !status || (DENSE ? !dense : (!packed || !area))) return S6D_EINVAL;
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(rle_status_init_kernel, dim3(1), dim3(1), 0, s, status);
  hipLaunchKernelGGL(rle_check_kernel, dim3((unsigned)N), dim3(RLE_THREADS), 0, s, counts, offsets, ends, R, pl.HW, area, status);
  if (!DENSE && !rle_words_owned(pl, W) && hipMemsetAsync(packed, 0, (size_t)N * pl.words * 8, s) != hipSuccess) return S6D_ELAUNCH;
  hipLaunchKernelGGL(rle_decode_kernel<DENSE>, dim3((unsigned)((long)N * pl.bands)), dim3(RLE_THREADS), 0, s, offsets, ends, H, W,
                     pl.pitch, pl.bc, pl.bands, pl.row_words, pl.words, status, (u64 *)packed, area, dense);
  return launch_status();
}

}  // namespace s6d

using namespace s6d;

extern "C" int s6d_set_rle_band_words(int words) {
  if (words < 0 || words > RLE_LDS_WORDS) return S6D_EINVAL;
  g_s6d_rle_band_words = words;
  return S6D_OK;
}

extern "C" long s6d_rle_encode_workspace_bytes(int N, int H, int W) {
  RlePlan pl;
  if (rle_plan(N, H, W, &pl) != S6D_OK) return -1;
  return (long)N * pl.ebands * 4 + 4;
}

extern "C" int s6d_rle_count_u8(const uint8_t *masks, int N, int H, int W, void *workspace, int32_t *run_counts, void *stream) {
  RlePlan pl;
  const int rc = rle_plan(N, H, W, &pl);
  if (rc != S6D_OK) return rc;
  if (N == 0) return S6D_OK;
  if (!masks || !workspace || !run_counts) return S6D_EINVAL;
  hipStream_t s = as_stream(stream);
  int *band_counts = reinterpret_cast<int *>(workspace);
  hipLaunchKernelGGL(rle_encode_kernel<false>, dim3((unsigned)((long)N * pl.ebands)), dim3(RLE_THREADS), 0, s, masks, H, W, pl.nw,
                     pl.pitch, pl.ec, pl.ebands, band_counts, (const long *)nullptr, 0L, (int *)nullptr);
  hipLaunchKernelGGL(rle_runs_kernel, dim3((unsigned)((N + RLE_THREADS - 1) / RLE_THREADS)), dim3(RLE_THREADS), 0, s, band_counts, N,
                     pl.ebands, run_counts);
  return launch_status();
}

extern "C" int s6d_rle_write_u8(const uint8_t *masks, int N, int H, int W, void *workspace, const long *offsets, long R,
                                int32_t *edges, int32_t *counts, void *stream) {
  RlePlan pl;
  const int rc = rle_plan(N, H, W, &pl);
  if (rc != S6D_OK) return rc;
  if (R < N) return S6D_EINVAL;
  const long blocks = (R + RLE_THREADS - 1) / RLE_THREADS;
  if (blocks > 0x7fffffffL) return S6D_EUNSUPPORTED;
  if (N == 0) return S6D_OK;
  if (!masks || !workspace || !offsets || !edges || !counts) return S6D_EINVAL;
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(rle_encode_kernel<true>, dim3((unsigned)((long)N * pl.ebands)), dim3(RLE_THREADS), 0, s, masks, H, W, pl.nw,
                     pl.pitch, pl.ec, pl.ebands, reinterpret_cast<int *>(workspace), offsets, R, edges);
  hipLaunchKernelGGL(rle_diff_kernel, dim3((unsigned)blocks), dim3(RLE_THREADS), 0, s, offsets, N, R, (int)pl.HW, edges, counts);
  return launch_status();
}

extern "C" int s6d_rle_to_packed(const int32_t *counts, const long *offsets, const long *ends, int N, long R, int H, int W,
                                 int32_t *status, uint64_t *packed, int32_t *area, void *stream) {
  return rle_decode<false>(counts, offsets, ends, N, R, H, W, status, packed, area, nullptr, stream);
}

extern "C" int s6d_rle_to_masks_u8(const int32_t *counts, const long *offsets, const long *ends, int N, long R, int H, int W,
                                   int32_t *status, uint8_t *masks, void *stream) {
  return rle_decode<true>(counts, offsets, ends, N, R, H, W, status, nullptr, nullptr, masks, stream);
}
