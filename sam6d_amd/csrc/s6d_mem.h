// The memory-side vocabulary of the LDS-DMA kernels of libsam6d_hip.so (gfx950): address-space qualifiers, counted waits, the 16-byte
// LDS-DMA issue in its two forms, the register pin and the dynamic-LDS declaration.  A kernel file uses these and spells none of them
// out itself.  Each entry states next to its device form what it is on the tests' host emulator (tests/hipemu.py, HIPEMU): this
// header and S6D_WAVE_RENDEZVOUS of csrc/s6d_common.h are the only places of csrc/ that name the emulator.
#pragma once
#include <hip/hip_runtime.h>

// Address spaces.  The emulator's compiler carries the LDS and global qualifiers as plain numbered address spaces; a constant-space
// pointer (uniform address + constant address space = s_load: lgkmcnt, not vmcnt) is a plain pointer there.
#define S6D_LDS(T) __attribute__((address_space(3))) T
#define S6D_GLOBAL(T) __attribute__((address_space(1))) T
#ifdef HIPEMU
#define S6D_CONST(T) T
#else
#define S6D_CONST(T) __attribute__((address_space(4))) T
#endif

// Counted waits: at most n vector-memory operations of this wave (LDS-DMA pieces among them) still in flight; every LDS / scalar-memory
// operation done.  n is a literal.  Emulator: the wave's pending LDS-DMAs beyond the youngest n land (hipemu::vmcnt_wait); LDS
// operations complete at once there, so the second wait is nothing.
#ifdef HIPEMU
#define S6D_VMCNT(n) hipemu::vmcnt_wait(n)
#define S6D_LGKM0() do { } while (0)
#else
#define S6D_VMCNT(n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")
#define S6D_LGKM0() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
#endif

// Register pin: an empty asm that makes the vector register(s) of x opaque at this point.  An MFMA is a pure register operation:
// neither s_barrier nor sched_barrier orders it at instruction-selection time (it has no chain), so a matrix segment is tied down by
// data -- operands pinned after the opening barrier (no MFMA can be placed above it), accumulators before the closing one (none can
// sink below it); the same pin keeps a value from being hoisted out of a loop.  Emulator: nothing.
#ifdef HIPEMU
#define S6D_PIN(x) do { } while (0)
#else
#define S6D_PIN(x) asm volatile("" : "+v"(x))
#endif

// A kernel's dynamic LDS, at namespace or at block scope.  Emulator: one block runs at a time, so every name, in whichever unit or
// namespace, is a reference to ONE host buffer of a CU's 160 KiB, defined right here (an inline variable: one object for the whole
// emulator library) -- the emulator's build step and runtime know nothing about the kernels' LDS arrays.
#ifdef HIPEMU
namespace s6d {
alignas(64) inline char emu_dyn_lds[160 * 1024];
}
#define S6D_DYN_LDS(name) static char (&name)[sizeof(::s6d::emu_dyn_lds)] = ::s6d::emu_dyn_lds
#else
#define S6D_DYN_LDS(name) extern __shared__ __attribute__((aligned(16))) char name[]
#endif

namespace s6d {

// One 1-KiB LDS-DMA piece: lane l's 16 bytes at src -> LDS byte address dst + 16 l (dst wave-uniform); counted by vmcnt.  Emulator:
// the same builtin, modelled by tests/host_cc/hipemu (the piece lands at the wait that covers it).
__device__ __forceinline__ void lds_dma16(const void *src, S6D_LDS(char) *dst) {
  __builtin_amdgcn_global_load_lds((const S6D_GLOBAL(void) *)src, dst, 16, 0, 0);
}

// The same piece issued as inline asm (the attention kernels' ring loops): with the builtin in the loop hipcc puts an
// s_waitcnt vmcnt(0) in front of the next LDS read -- the first ds_read_b64_tr_b16 of every tile; it cannot tell that the reads touch
// another ring slot -- which drains the look-ahead, so the prefetch never overlaps the arithmetic (docs/NOTEBOOK_r1_r4.md section 4.2,
// profiles/r04_win16_dma_waits.txt); the waits of those kernels are the counted ones they write out.  M0 is on the clobber list (the
// library is built with -Wno-inline-asm: hipcc warns about reserved registers there); nothing else in those kernels uses it.
// Emulator: the builtin form.
__device__ __forceinline__ void lds_dma16_m0(const void *src, S6D_LDS(char) *dst) {
#ifdef HIPEMU
  lds_dma16(src, dst);
#else
  const unsigned a = __builtin_amdgcn_readfirstlane((unsigned)(size_t)dst);
  // s_nop: one wait state between the SALU write of M0 and the LDS-DMA that reads it (hipcc puts the same nop after its own s_mov m0)
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(src), "s"(a) : "memory", "m0");
#endif
}

}  // namespace s6d
