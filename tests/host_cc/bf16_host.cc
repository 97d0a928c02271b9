// Host build of sam6d_amd/csrc/s6d_bf16.h (tests/test_bf16_host.py): the header is compiled unchanged against the emulator's HIP
// header (tests/host_cc/hipemu) and its element helpers are called on arrays.  Build: clang++ -O2 -std=c++17 -I hipemu -I csrc.
#include "s6d_bf16.h"

extern "C" void bf16_bits_host(const float *x, long n, unsigned short *out) {
  for (long i = 0; i < n; ++i) out[i] = s6d::bf16_bits(x[i]);
}
extern "C" void bf16_value_host(const unsigned short *h, long n, float *out) {
  for (long i = 0; i < n; ++i) out[i] = s6d::bf16_value(h[i]);
}
extern "C" void bf16_split_host(const float *x, long n, unsigned short *hi, unsigned short *lo) {
  for (long i = 0; i < n; ++i) s6d::bf16_split(x[i], hi[i], lo[i]);
}
extern "C" int kswz_host(int row) { return s6d::kswz(row); }
