// gemm_fill.h -- helpers of gemm_nt_kernel's global -> LDS staging: the index sets of the fill cut in parts, and the register-staged
// gather of the A tile from pixels (im2col on load, ADDR 2 / 3).
#pragma once
#include "gemm_lds.h"

namespace plipmi {

// index sets of the staged fill: [p0, p1) without [g0, g1)
constexpr int count_outside(int p0, int p1, int g0, int g1) {
  int c = 0;
  for (int i = p0; i < p1; ++i) c += (i >= g0 && i < g1) ? 0 : 1;
  return c;
}
constexpr int nth_outside(int p0, int p1, int g0, int g1, int k) {
  for (int i = p0; i < p1; ++i) {
    if (i >= g0 && i < g1) continue;
    if (k == 0) return i;
    --k;
  }
  return p0;
}

// ADDR 2 helpers (im2col on load): a 16-byte pixel load into registers that hipcc does not count, and the wait that hands the
// registers back to it -- they pass THROUGH the wait statement, so no use of them is scheduled above it (cdna_hip_programming.md
// 5.7 item 1, VGPR destinations, form ii).  s_nop 4: the scalar offset may come straight from SALU arithmetic.
__device__ __forceinline__ void pix_load16(u32x4& dst, unsigned voff, const i32x4 rsrc, unsigned soff) {
  asm volatile("s_nop 4\n\tbuffer_load_dwordx4 %0, %1, %2, %3 offen" : "=v"(dst) : "v"(voff), "s"(rsrc), "s"(soff) : "memory");
}
// (the count is chosen by a wave-uniform branch around OPERAND-FREE wait statements; the registers then pass through ONE
//  unconditional empty statement behind them -- a register-tied statement on each side of a branch makes hipcc merge the two
//  register sets with v_mov copies in FRONT of the waits, i.e. it reads the destinations before the data has landed)
__device__ __forceinline__ void tie_regs5(u32x4& a, u32x4& b, u32x4& c, u32x4& d, u32x4& e) {
  asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e) : : "memory");
}
// ADDR 3: twelve bytes = four RGB pixels of a uint8 tile
typedef __attribute__((ext_vector_type(3))) unsigned u32x3;
__device__ __forceinline__ void pix_load12(u32x3& dst, unsigned voff, const i32x4 rsrc, unsigned soff) {
  asm volatile("s_nop 4\n\tbuffer_load_dwordx3 %0, %1, %2, %3 offen" : "=v"(dst) : "v"(voff), "s"(rsrc), "s"(soff) : "memory");
}
__device__ __forceinline__ void tie_regs5(u32x3& a, u32x3& b, u32x3& c, u32x3& d, u32x3& e) {
  asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e) : : "memory");
}
// CLIP normalisation of a byte of channel c as one fma: A_c = fl((1 / std_c) / 255), B_c = fl(-mean_c / std_c)  (bit patterns, so that no
// compiler's constant folding can move them)
__device__ __forceinline__ float u8_norm(float b, int c) {
  const unsigned A[3] = {0x3c6f2e3cu, 0x3c75e324u, 0x3c68fb47u}, Bc[3] = {0xbfe568dbu, 0xbfe044b8u, 0xbfbd77d7u};
  return fmaf(b, __builtin_bit_cast(float, A[c]), __builtin_bit_cast(float, Bc[c]));
}

}  // namespace plipmi
