// 16-bit element helpers shared by the kernel files of libsam6d_hip.so (gfx950): the vector types of the matrix instructions, the
// fp32 <-> bf16 conversion pair, the hi / lo split behind every fp32-class product of the PEM, and the LDS chunk swizzle.  Every
// csrc/*.hip is its own translation unit in namespace s6d: a kernel file includes this header and defines none of these itself.
#pragma once
#include "s6d_common.h"
#include "s6d_mem.h"

namespace s6d {

typedef unsigned short u16;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;   // f32x2 and f32x4 are s6d_common.h's: its gelu_erf4 needs them
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(4))) short s16x4;

// fp32 -> the bits of the nearest bf16, ties to even, NaN stays NaN (v_cvt_pk_bf16_f32 on gfx950), and back (exact).  The names say
// bf16 on purpose: csrc/s6d_attn_common.h has f2bf / bf2f for "the element type of this build", which is IEEE half in one of its two
// builds.  (csrc/s6d_norm.hip keeps an integer-rounding f2bf_ of its own: see there.)
__device__ __forceinline__ u16 bf16_bits(float f) {
  union { __bf16 b; u16 u; } x;
  x.b = (__bf16)f;
  return x.u;
}
__device__ __forceinline__ float bf16_value(u16 h) { return __uint_as_float(((unsigned)h) << 16); }

// x = hi + lo in bf16, hi = bf16(x), lo = bf16(x - hi): |x - (hi + lo)| <= 2^-16 |x| (two roundings of 2^-8 relative each).  The
// fp32-class products on the bf16 matrix cores (plin / pchain / pe, geo / fine / ism) multiply such pairs in three terms,
// a_hi b_hi + a_lo b_hi + a_hi b_lo with fp32 accumulation: ~2^-17 relative per product.  The ORDER of the three matrix instructions
// belongs to the kernel family and is not part of this header.
__device__ __forceinline__ void bf16_split(float x, u16 &hi, u16 &lo) {
  const u16 h = bf16_bits(x), l = bf16_bits(x - bf16_value(h));    // both before either store: hi may live in memory
  hi = h;
  lo = l;
}

// LDS images read with ds_read_b128 (one 16-byte chunk per lane, 16 rows per lane group): rows whose (row >> 2 ^ row >> 3) & 1 is
// set keep their 16-byte chunks pairwise swapped.  The two row sets of a lane group ({0-3,12-15} reading chunk g, {4-11} reading
// chunk g + 1) otherwise meet on bank slots whenever the row stride is an odd number of chunks: 5 of 16 slots at 13 chunks (the
// attention K images), 3 of 16 at 5 chunks (the 80-byte rows of plin / geo) -- a 2-way conflict on every fragment read.  The writer
// stores chunk c of row r at c ^ kswz(r), the reader asks for its chunk the same way.
__device__ __forceinline__ int kswz(int row) { return ((row >> 2) ^ (row >> 3)) & 1; }

}  // namespace s6d
