// attention_mfma_dev.h -- the device code the MFMA attention kernels share (attention_mfma.hip: the single-pass kernel for
// S <= 128 and the two chunked online-softmax kernels; qkv_attention.hip: the attention in the fused text kernel's epilogue): the LDS
// images of Q / K / V and the steps that turn them into normalised output rows of one block of 32 queries -- fragment reads,
// mask, P V product, output staging (the products and their layouts: attention_mfma.hip's header comment).  Kernels built from
// these functions perform the same operations in the same order per query, so they produce the same bits.  Staging, barriers, the
// live / open tile tests, the exp pass and the LOOPS stay with each kernel: a function here is one step on values (one fragment,
// one MFMA, one store) -- helpers that held the ks / dt / q4 loops changed the kernels' instructions (profiles/attention_shared_isa.txt);
// what the two chunked kernels share beyond these steps, their online-softmax update, is text for that reason: attention_flash_step.inc.
// A wave works on 32 queries: lane = query lrow = lane & 31, half hi = lane >> 5; lsw = (lrow >> 1) & 7 is the swizzle term of
// the lane's row in any block or tile that starts at a multiple of 16 rows.
#pragma once
#include "gemm_lds.h"
#include "kernels.h"

namespace plipmi {
namespace attn_dev {

typedef __attribute__((ext_vector_type(4))) short i16x4;

constexpr float kLog2e = 1.4426950408889634f;   // exp(x - m) = 2^(x log2 e - m log2 e): one FMA + v_exp_f32 per score

// ---- LDS images: address of the 16-byte piece `chunk` (8 head-dim columns) of `row`.  Q and K (and the output tile, which reuses
// their rows): 128-byte rows with the GEMM's XOR swizzle, so the fragment ds_read_b128 -- 32 rows, one chunk -- are conflict-free.
template <typename C>
__device__ __forceinline__ C* k_image(C* img, int row, int chunk) { return img + row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }
// V stays row-major (whole 16-byte pieces straight from the rows) as two [keys][32 columns] images, one per 32-wide head-dim
// tile, 64-byte rows, vimg bytes apart.  vimg = rows * 64 + 64 starts the second image 64 bytes past a 128-byte boundary: the
// eight 16-byte pieces of one V row (four per image) then cover all 32 write banks once instead of hitting the same 16 twice
// (SQ_LDS_BANK_CONFLICT, round 1: half of the 3.9e5 conflict cycles per launch; the other half was the output staging below).
template <typename C>
__device__ __forceinline__ C* v_image(C* img, int row, int chunk, int vimg) { return img + (chunk >> 2) * vimg + row * 64 + (chunk & 3) * 16; }

// ds_read_b64_tr_b16 hands lane (d = lane&31, g = lane>>5) the four keys k0+4g .. k0+4g+3 of column d of a V image -- exactly one
// half of the V^T MFMA fragment under the key permutation of the score accumulator -- with every 32-lane half of the instruction
// touching each of the 64 banks once (4 rows x 64 B).
// Per-lane byte offset inside an image; the (tile, sub-block, image) terms are compile-time immediates.
__device__ __forceinline__ int vtr_lane_offset(int lrow, int hi) {
  return (((lrow & 15) >> 2) + 4 * hi) * 64 + ((lrow & 3) * 4 + (lrow >> 4) * 16) * 2;
}
template <typename H>
__device__ __forceinline__ typename half_traits<H>::x8 vtr_fragment(const char* vs, int byte_off) {
  typedef __attribute__((address_space(3))) i16x4* lds_ptr;
  const i16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(vs + byte_off));
  const i16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(vs + byte_off + 8 * 64));  // keys +8
  typedef __attribute__((ext_vector_type(8))) short i16x8;
  const i16x8 v = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  return __builtin_bit_cast(typename half_traits<H>::x8, v);
}

// ---- scores^T = K Q^T: mma16<HT>(sc, K fragment, Q fragment) over ks = 0 .. 3 (gemm_lds.h).  The lane's 16 bytes of row `row` of
// a Q or K image for step ks, columns 16 ks + 8 hi .. + 7: A operand from K row 32 t + lrow of key tile t, B operand from Q row q0 + lrow.
__device__ __forceinline__ u32x4 image_fragment(const char* img, int row, int ks, int hi, int lsw) {
  return *reinterpret_cast<const u32x4*>(img + row * 128 + (((ks * 2 + hi) ^ lsw) << 4));
}

// ---- mask
// The keys a lane may use in a tile are ONE 32-bit word: validity (padding / attention_mask) AND, under the causal mask,
// causal_bits(d): keys 32 t + j <= query  <=>  j <= d = query - 32 t.
__device__ __forceinline__ unsigned causal_bits(int d) { return d < 0 ? 0u : (d >= 31 ? 0xffffffffu : (2u << d) - 1u); }
// Slot r of the accumulator holds key 32 t + 4 hi + (r&3) + 8 (r>>2): after a shift by 4 hi its bit sits at a compile-time
// position, so masking a score is a 1-bit field extract (0 / -1), an AND that turns it into 0.0 / -inf, and an add -- no compares,
// no 64-bit shifts, no branches.  (The two-operation form, a bit select against -inf, was miscompiled by this hipcc: its
// v_bitop3_b32 folding mixed the elements' masks.)  The maximum of the masked scores is folded into running_max.
__device__ __forceinline__ void mask_scores(f32x16& sc, unsigned bits, int hi, float& running_max) {
  const unsigned nbits = ~(bits >> (4 * hi));        // 1 = masked
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const unsigned m = (unsigned)__builtin_amdgcn_sbfe((int)nbits, (r & 3) + 8 * (r >> 2), 1);   // masked ? 0xffffffff : 0
    sc[r] += __builtin_bit_cast(float, m & 0xff800000u);                                          // + (-inf) or + 0
    running_max = fmaxf(running_max, sc[r]);
  }
}
// an open tile -- every query of the wave may use every key of it: nothing to mask, the maximum alone
__device__ __forceinline__ void max_scores(const f32x16& sc, float& running_max) {
#pragma unroll
  for (int r = 0; r < 16; ++r) running_max = fmaxf(running_max, sc[r]);
}

// ---- O^T = V^T P^T
// The P operand of keys 16 s2 .. 16 s2 + 15 of a tile: its probabilities rounded to the operand type, a plain register pack --
// the accumulator's key permutation is the one vtr_fragment reads V in.
template <typename HT>
__device__ __forceinline__ typename half_traits<HT>::x8 pack_p(const f32x16& sc, int s2) {
  typename half_traits<HT>::x8 pf;
#pragma unroll
  for (int jj = 0; jj < 8; ++jj) pf[jj] = (HT)sc[8 * s2 + jj];
  return pf;
}
// acc + V^T P^T over the 16 keys key0 .. key0 + 15 for head-dim tile dt; vlane = the lane's address in the first V image
template <typename HT>
__device__ __forceinline__ f32x16 pv_step(const char* vlane, int vimg, int dt, int key0, typename half_traits<HT>::x8 pf, f32x16 acc) {
  return half_traits<HT>::mfma32(vtr_fragment<HT>(vlane, dt * vimg + key0 * 64), pf, acc);
}

// ---- output: the accumulator layout gives a lane one query ROW (like the GEMM).  The normalised 32 x 64 tile goes into rows of a
// Q / K image that the wave owns by then (transposing ds_write_b64, orow_lds = the lane's row); whole 128-byte rows then go to memory.
// XCHG: rows 2k and 2k+1 share a swizzle slot; odd rows keep their two 8-byte halves exchanged, so the 16 lanes of a
// ds_write_b64 group (16 consecutive rows, same column chunk) touch 16 distinct 8-byte bank pairs.  load_out_row undoes it.
// One store: the four columns d = 32 dt + 8 q4 + 4 hi .. + 3 of the row, acc = the accumulator of head-dim tile dt.
template <typename HT, bool XCHG>
__device__ __forceinline__ void stage_out4(char* orow_lds, int lrow, int hi, int lsw, int dt, int q4, const f32x16& acc, float inv) {
  using X4 = typename half_traits<HT>::x4;
  const int d = dt * 32 + 8 * q4 + 4 * hi;
  const int c = d >> 3;                                    // 16-byte chunk, half (d&4) inside it
  const X4 v = {from_f32<HT>(acc[4 * q4 + 0] * inv), from_f32<HT>(acc[4 * q4 + 1] * inv),
                from_f32<HT>(acc[4 * q4 + 2] * inv), from_f32<HT>(acc[4 * q4 + 3] * inv)};
  if (XCHG) *reinterpret_cast<X4*>(orow_lds + ((c ^ lsw) << 4) + ((((d >> 2) ^ lrow) & 1) << 3)) = v;
  else *reinterpret_cast<X4*>(orow_lds + ((c ^ lsw) << 4) + (d & 4) * 2) = v;
}
// piece `chunk` of output row `row`, as it goes to memory
template <bool XCHG>
__device__ __forceinline__ u32x4 load_out_row(const char* img, int row, int chunk) {
  const u32x4 raw = *reinterpret_cast<const u32x4*>(k_image(img, row, chunk));
  return (XCHG && (row & 1)) ? u32x4{raw[2], raw[3], raw[0], raw[1]} : raw;
}

}  // namespace attn_dev
}  // namespace plipmi
