// In-order compaction of a workgroup's elements (wave ballot ranks + a 16-entry wave prefix): shared by the PEM pre-processing
// (s6d_pempre.hip) and the template onboarding (s6d_onboard.hip).
#pragma once
#include "s6d_common.h"

namespace s6d {

constexpr int kCmpThreads = 1024;

// in-order compaction step of one 1024-element chunk: returns this lane's output position (or -1) and advances *base
__device__ __forceinline__ long block_rank(bool keep, long *base, unsigned *wave_tot) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long bal = __ballot(keep);
  const int rank = __popcll(bal & ((1ull << lane) - 1ull));
  if (lane == 0) wave_tot[wave] = (unsigned)__popcll(bal);
  __syncthreads();
  long off = *base;
  unsigned tot = 0;
  for (int w = 0; w < kCmpThreads / 64; ++w) {
    if (w < wave) off += wave_tot[w];
    tot += wave_tot[w];
  }
  __syncthreads();                                      // everyone has read base / wave_tot before they change
  if (tid == 0) *base += tot;
  return keep ? off + rank : -1;
}

}  // namespace s6d
