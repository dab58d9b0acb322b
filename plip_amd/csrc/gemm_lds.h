// gemm_lds.h -- LDS-DMA, write-through store and MFMA helpers of the GEMM kernels (gemm_kernel.h, gemm_skinny.hip,
// qkv_attention.hip); attention_mfma_dev.h takes the vector types and mma16 from here.
#pragma once
#include "common.h"

namespace plipmi {

// first-class vector (HIP's uint4 struct keeps staging arrays in scratch)
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;

// LDS-DMA (global_load_lds_dwordx4): each lane's 16 bytes at `gsrc` land at
// `lds_wave_base + lane*16` (wave-uniform base in M0).  Issued through inline asm
// on purpose: with the builtin, hipcc cannot tell that the DMA fills the OTHER
// LDS buffer and drains it (s_waitcnt vmcnt(0)) in front of the first ds_read of
// the current one, which serialises load and compute.  The asm form is invisible
// to its wait-count pass; the kernel waits vmcnt(0) itself right before the barrier
// that publishes the buffer (cdna_hip_programming.md 5.7 item 1).  M0 is saved and
// restored inside the statement because the compiler owns it.
__device__ __forceinline__ void glds16(const char* gsrc, unsigned lds_wave_base) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(gsrc), "s"(lds_wave_base)
      : "memory");
}
// The same LDS-DMA through the buffer path: a 128-bit resource descriptor in SGPRs (base, size) plus ONE 32-bit
// per-lane byte offset instead of a 64-bit per-lane address (ADDR = 1 kernels).
typedef __attribute__((ext_vector_type(4))) int i32x4;
__device__ __forceinline__ i32x4 make_buffer_rsrc(const void* base) {
  const unsigned long long a = (unsigned long long)base;
  i32x4 r;
  r[0] = __builtin_amdgcn_readfirstlane((int)(a & 0xffffffffull));
  r[1] = __builtin_amdgcn_readfirstlane((int)((a >> 32) & 0xffffull));  // stride 0: raw buffer
  r[2] = -1;                                                              // num_records: whole address range
  r[3] = 0x00020000;                                                      // gfx9-family raw dword buffer
  return r;
}
// soff: wave-uniform byte offset (the K position) in an SGPR -- the per-lane offsets never change inside the K loop
__device__ __forceinline__ void glds16_buf(const i32x4 rsrc, unsigned voff, unsigned soff, unsigned lds_wave_base) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(rsrc), "s"(soff), "s"(lds_wave_base)
      : "memory");
}
// N pieces under ONE M0 save/restore; the LDS destination of piece e is lds_base + OFFe (compile-time), formed by
// the s_add that writes M0.  Operand order per piece: resource, lane offset.
template <int N, int OFF0, int OFF1 = 0, int OFF2 = 0, int OFF3 = 0>
__device__ __forceinline__ void glds16_buf_n(unsigned lds_base, unsigned soff, const i32x4 r0, unsigned v0,
                                             const i32x4 r1, unsigned v1, const i32x4 r2, unsigned v2,
                                             const i32x4 r3, unsigned v3) {
  unsigned keep;
  if constexpr (N == 1) {
    asm volatile("s_mov_b32 %0, m0\n\t"
                 "s_add_u32 m0, %1, %4\n\ts_nop 0\n\tbuffer_load_dwordx4 %3, %2, %5 offen lds\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(keep) : "s"(lds_base), "s"(r0), "v"(v0), "i"(OFF0), "s"(soff) : "memory", "scc");
  } else if constexpr (N == 2) {
    asm volatile("s_mov_b32 %0, m0\n\t"
                 "s_add_u32 m0, %1, %6\n\ts_nop 0\n\tbuffer_load_dwordx4 %3, %2, %8 offen lds\n\t"
                 "s_add_u32 m0, %1, %7\n\ts_nop 0\n\tbuffer_load_dwordx4 %5, %4, %8 offen lds\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(keep) : "s"(lds_base), "s"(r0), "v"(v0), "s"(r1), "v"(v1), "i"(OFF0), "i"(OFF1), "s"(soff)
                 : "memory", "scc");
  } else if constexpr (N == 3) {
    asm volatile("s_mov_b32 %0, m0\n\t"
                 "s_add_u32 m0, %1, %8\n\ts_nop 0\n\tbuffer_load_dwordx4 %3, %2, %11 offen lds\n\t"
                 "s_add_u32 m0, %1, %9\n\ts_nop 0\n\tbuffer_load_dwordx4 %5, %4, %11 offen lds\n\t"
                 "s_add_u32 m0, %1, %10\n\ts_nop 0\n\tbuffer_load_dwordx4 %7, %6, %11 offen lds\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "s"(lds_base), "s"(r0), "v"(v0), "s"(r1), "v"(v1), "s"(r2), "v"(v2), "i"(OFF0), "i"(OFF1), "i"(OFF2), "s"(soff)
                 : "memory", "scc");
  } else {
    asm volatile("s_mov_b32 %0, m0\n\t"
                 "s_add_u32 m0, %1, %10\n\ts_nop 0\n\tbuffer_load_dwordx4 %3, %2, %14 offen lds\n\t"
                 "s_add_u32 m0, %1, %11\n\ts_nop 0\n\tbuffer_load_dwordx4 %5, %4, %14 offen lds\n\t"
                 "s_add_u32 m0, %1, %12\n\ts_nop 0\n\tbuffer_load_dwordx4 %7, %6, %14 offen lds\n\t"
                 "s_add_u32 m0, %1, %13\n\ts_nop 0\n\tbuffer_load_dwordx4 %9, %8, %14 offen lds\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "s"(lds_base), "s"(r0), "v"(v0), "s"(r1), "v"(v1), "s"(r2), "v"(v2), "s"(r3), "v"(v3), "i"(OFF0), "i"(OFF1),
                   "i"(OFF2), "i"(OFF3), "s"(soff)
                 : "memory", "scc");
  }
}
__device__ __forceinline__ void wait_vm0() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// One 16-byte chunk of K per lane -> one (16-bit operand types) or four (fp32) MFMAs.
template <typename T>
__device__ __forceinline__ void mma16(f32x16& acc, const u32x4& wfrag, const u32x4& xfrag) {
  if constexpr (sizeof(T) == 2) {
    using X8 = typename half_traits<T>::x8;
    acc = half_traits<T>::mfma32(__builtin_bit_cast(X8, wfrag), __builtin_bit_cast(X8, xfrag), acc);
  } else {
    // lane group g = lane>>5 holds k = 4*(2*kq+g)+j, j=0..3, for BOTH operands, so
    // MFMA j multiplies matching k's (any k permutation shared by A and B is valid).
    f32x4 w = __builtin_bit_cast(f32x4, wfrag), x = __builtin_bit_cast(f32x4, xfrag);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w[j], x[j], acc, 0, 0, 0);
  }
}

// 16-byte output store, written THROUGH the XCD's L2 (sc0 sc1): the line goes to the fabric now, while other workgroups
// are still in their K loops, instead of staying dirty until the end-of-kernel write-back every launch otherwise ends with
// (MI355X_MICROARCH.md, "boundary": + B / 6 TB/s for B dirty bytes): -0.5 ... -4 us per launch on the eight production
// shapes against plain stores (profiles/r03_gemm_tiles.txt, measured while a process-wide switch existed: commit ba1f4b8;
// as a run-time flag the choice itself cost 1 % of the two-stream step).  The asm store ends with s_nop 1: hipcc does not
// know the statement reads its data registers after issue (cdna_hip_programming.md 5.7 item 1).
__device__ __forceinline__ void store16(void* ptr, const u32x4 v) {
  asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"(ptr), "v"(v) : "memory");
}

}  // namespace plipmi
