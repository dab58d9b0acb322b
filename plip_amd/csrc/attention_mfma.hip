// attention_mfma.hip -- MFMA attention for the two 16-bit engines (bf16 / f16).  Short CLIP sequences (S <= 128: 50 vision tokens, 77 text tokens)
// take the single-pass kernel: one workgroup per (image|caption, head), one wavefront per block of 32 queries,
// v_mfma_f32_32x32x16_bf16 / _f16 for both products.  Longer ones (ViT-B/16, ViT-L/14[@336]) take the chunked
// online-softmax kernel further down; heads of 72 .. 128 take the padded chunked kernel behind it, whatever the length.  All of
// them, and the fused text kernel of qkv_attention.hip, take the LDS images, the fragment reads, the mask, the P V step and the
// output staging from attention_mfma_dev.h, where they are written once; the two chunked kernels share their online-softmax step
// (attention_flash_step.inc).
//
//   scores^T = K Q^T   (operands swapped): a lane owns ONE query column (lane&31) and
//                      16 keys per 32-key tile, so the softmax row reductions are a
//                      register max/sum plus one exchange with lane^32 -- no LDS.
//   O^T = V^T P^T      the contraction index (key) may be permuted freely as long as
//                      both MFMA operands use the same permutation.  Choosing the
//                      permutation that the QK^T accumulator layout already has
//                      (slot jj of lane group g  <->  key (jj&3) + 4g + 8(jj>>2) + 16s)
//                      makes the P operand a plain register pack: no cross-lane shuffle.
//                      V^T comes from a row-major LDS copy of V through the hardware transpose read
//                      ds_read_b64_tr_b16 (two [keys][32] images with 64-byte rows -> conflict-free).
//   Softmax statistics, the running sum and the 1/l normalisation are fp32
//   (modeling_clip.py:271); P is rounded to the operand type only as the MFMA operand.
#include "attention_mfma_dev.h"
#include "dispatch.h"
#include "kernels.h"

namespace plipmi {

using namespace attn_dev;

// One (sample, head) problem per workgroup.  (Two problems per workgroup with a register prefetch of the next K / V rows
// was measured slower in round 2 -- registers: three waves per SIMD instead of six to eight -- and is gone.)
// (amdgpu_waves_per_eu(4, 4): with the default heuristics hipcc parks the MFMA accumulators in AGPRs and pays 96 v_accvgpr
// copies per wave to get the scores and the outputs back into VGPRs; told it may use 128 registers it needs 77 (S <= 64) / 93
// (S <= 96) plain VGPRs, no AGPRs, 10-12 % fewer VALU instructions, and one more wave per SIMD than before.)
template <typename HT, int KT>  // 32-key tiles: S <= 32*KT
__global__ __launch_bounds__(64 * KT) __attribute__((amdgpu_waves_per_eu(4, 4))) void attention_mfma_kernel(const HT* __restrict__ qkv, HT* __restrict__ out, int S, int H,
                                                                 int causal, const int64_t* __restrict__ key_mask,
                                                                 const int* __restrict__ cu /* packed rows: sample b owns rows
                                                                 cu[b] .. cu[b+1]-1 of qkv / out (nullptr: b*S .. b*S+S-1) */) {
  using X8 = typename half_traits<HT>::x8;
  constexpr int SP = 32 * KT;   // padded sequence
  constexpr int NT = 64 * KT;
  constexpr int NP = SP * 8 / NT;   // 16-byte pieces of K (and of V) per thread: 4
  // K rows are staged through LDS in whole 128-byte lines (8 lanes x 16 B per row) instead of being loaded
  // fragment-shaped (16 B from each of 32 rows per instruction, which costs the texture-address unit 2x the
  // time for the same bytes); the LDS image uses the GEMM's XOR swizzle so the fragment ds_read_b128 are
  // conflict-free.  V keeps its row-major form (two [SP][32] images) and is transposed by the LDS read itself.
  constexpr int VIMG = SP * 64 + 64;   // v_image: the second image 64 bytes past a 128-byte boundary
  __shared__ __attribute__((aligned(16))) char Ks[SP * 128];
  __shared__ __attribute__((aligned(16))) char Vs[2 * VIMG];
  __shared__ unsigned long long mk[4];

  const int D = H * 64, ld = 3 * D;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q0 = wave * 32;
  const int lrow = lane & 31, hi = lane >> 5;
  const int qidx = q0 + lrow;
  const int lsw = (lrow >> 1) & 7;
  const int bh = blockIdx.x;

  u32x4 kreg[NP], vreg[NP];
  {
    const int b = bh / H, h = bh - b * H;
    // packed captions: this problem's rows start at cu[b] and there are cu[b+1] - cu[b] of them (queries AND keys); the
    // tokenizer mask keeps its [B, S] layout.  Keys past the caption's last row are masked like sequence padding, so a
    // query's result is the one the padded layout gives it, bit for bit (a masked key contributes an exact zero).
    const int row0 = __builtin_amdgcn_readfirstlane(cu ? cu[b] : b * S);
    const int Sb = __builtin_amdgcn_readfirstlane(cu ? cu[b + 1] - row0 : S);
    const bool active = q0 < Sb;
    const HT* base = qkv + (size_t)row0 * ld + h * 64;
#pragma unroll
    for (int i = 0; i < NP; ++i) {   // this thread's 16-byte pieces of the problem's K and V rows -> registers
      const int e = tid + i * NT, row = e >> 3, c = e & 7;
      // wave-uniform base + 32-bit lane offset (a problem spans < 4 GiB): scalar-base global loads, no 64-bit lane arithmetic
      const unsigned off = ((unsigned)(row < Sb ? row : Sb - 1) * (unsigned)ld + (unsigned)(c * 8)) * (unsigned)sizeof(HT);
      kreg[i] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(base + D) + off);
      vreg[i] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(base + 2 * D) + off);
    }
    // key validity bits (sequence padding and the tokenizer's attention_mask): key = tid
    {
      const bool ok = tid < Sb && (key_mask == nullptr || key_mask[(size_t)b * S + tid] != 0);
      const unsigned long long bits = __ballot(ok);
      if (lane == 0) mk[wave] = bits;
      if (KT < 4 && tid < 4 - KT) mk[KT + tid] = 0ull;
    }
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int e = tid + i * NT, row = e >> 3, c = e & 7;
      *reinterpret_cast<u32x4*>(k_image(Ks, row, c)) = kreg[i];
      *reinterpret_cast<u32x4*>(v_image(Vs, row, c, VIMG)) = vreg[i];
    }
    // Q fragments (B operand) straight from global memory: Q[query = lrow][d = 16ks + 8hi .. +7].  Only this wave reads
    // these rows, so an LDS image of Q would only cost residency (8-16 KB per workgroup = a third of its LDS).
    u32x4 qf[4];
    {
      const unsigned qoff = ((unsigned)(qidx < Sb ? qidx : Sb - 1) * (unsigned)ld + (unsigned)(hi * 8)) * (unsigned)sizeof(HT);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
        qf[ks] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(base) + qoff + ks * 16 * sizeof(HT));
    }
    __syncthreads();

    // scores^T tiles
    f32x16 sc[KT];
    // key validity words as scalars (wave-uniform): 32 keys per tile
    const unsigned long long m0 = mk[0], m1 = mk[1];
    const unsigned vw[4] = {(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)m0),
                            (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(m0 >> 32)),
                            (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)m1),
                            (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(m1 >> 32))};
    float rmax = -INFINITY;
#pragma unroll
    for (int t = 0; t < KT; ++t) {
      const bool live = active && !(causal && 32 * t > q0 + 31);  // wave-uniform: tile entirely above the diagonal
#pragma unroll
      for (int r = 0; r < 16; ++r) sc[t][r] = 0.f;
      if (live) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) mma16<HT>(sc[t], image_fragment(Ks, 32 * t + lrow, ks, hi, lsw), qf[ks]);
      }
      // (round 6) a tile every query of the wave may use entirely -- all 32 keys valid and, under the causal mask, wholly below the
      // diagonal: nothing to mask (wave-uniform test; the 50-token vision tower's first key tile is always one)
      if (live && vw[t] == 0xffffffffu && (!causal || 32 * t + 31 <= q0)) {
        max_scores(sc[t], rmax);
        continue;
      }
      unsigned bits = live ? vw[t] : 0u;   // the keys this lane may use in the tile: validity AND causal limit
      if (causal) {
        const int d = qidx - 32 * t;       // causal_bits(d), written out: the call changes this kernel's instructions
        bits &= d < 0 ? 0u : (d >= 31 ? 0xffffffffu : (2u << d) - 1u);
      }
      mask_scores(sc[t], bits, hi, rmax);
    }
    __syncthreads();  // every wave has its scores: the K rows may now be reused as output staging
    if (active) {
      rmax = fmaxf(rmax, __shfl_xor(rmax, 32, 64));
      const float m_use = (rmax == -INFINITY) ? 0.f : rmax;
      const float m2 = m_use * kLog2e;
      float rsum = 0.f;
#pragma unroll
      for (int t = 0; t < KT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          sc[t][r] = __builtin_amdgcn_exp2f(fmaf(sc[t][r], kLog2e, -m2));
          rsum += sc[t][r];
        }
      rsum += __shfl_xor(rsum, 32, 64);

      // O^T = V^T P^T
      f32x16 acc[2];
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[dt][r] = 0.f;
      const char* vlane = Vs + vtr_lane_offset(lrow, hi);
#pragma unroll
      for (int t = 0; t < KT; ++t) {
        if (causal && 32 * t > q0 + 31) continue;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          const X8 pf = pack_p<HT>(sc[t], s2);
#pragma unroll
          for (int dt = 0; dt < 2; ++dt) acc[dt] = pv_step<HT>(vlane, VIMG, dt, 32 * t + 16 * s2, pf, acc[dt]);
        }
      }
      // the normalised 32 x 64 tile into the K rows of the wave's own query range (every wave is past its scores), odd rows
      // with their halves exchanged, then whole 128-byte rows to memory
      const float inv = 1.0f / rsum;
      char* orow_lds = Ks + (q0 + lrow) * 128;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) stage_out4<HT, true>(orow_lds, lrow, hi, lsw, dt, q4, acc[dt], inv);
      __builtin_amdgcn_wave_barrier();
      const int c = lane & 7;
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int r = q0 + it * 8 + (lane >> 3);
        const u32x4 v = load_out_row<true>(Ks, r, c);
        if (r < Sb) *reinterpret_cast<u32x4*>(out + ((size_t)row0 + r) * D + h * 64 + c * 8) = v;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// S > 128 (ViT-B/16: 197 tokens, ViT-L/14: 257, ViT-L/14@336: 577): the same two MFMA products, streamed over
// 128-key chunks with an online softmax.  One workgroup = 128 queries of one (sample, head) (4 waves x 32), grid
// (B*H, ceil(S/128)).  Because a lane owns one query column in BOTH accumulator layouts (scores^T and O^T), the
// running max / running sum / rescale of the online softmax are per-lane scalars: no cross-lane traffic beyond the
// one lane^32 exchange per chunk.  K and V^T chunks are staged through LDS exactly like the short-sequence kernel.
// Round 4: the NEXT chunk's K / V rows travel global -> registers while the current chunk is multiplied (32 VGPRs of
// staging; the LDS write waits behind the chunk's barrier), so a workgroup no longer stands still for a global round trip
// per chunk; and the short kernel's per-score arithmetic -- one 32-bit mask word per tile, additive -inf, exp as FMA + v_exp_f32.
// ---------------------------------------------------------------------------------------------
template <typename HT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void attention_flash_kernel(const HT* __restrict__ qkv, HT* __restrict__ out,
                                                              int S, int H, int causal,
                                                              const int64_t* __restrict__ key_mask) {
  using X8 = typename half_traits<HT>::x8;
  constexpr int SP = 128;
  constexpr int NP = SP * 8 / 256;   // 16-byte pieces of a chunk's K (and V) rows per thread: 4
  __shared__ __attribute__((aligned(16))) char Qs[SP * 128];
  __shared__ __attribute__((aligned(16))) char Ks[SP * 128];
  __shared__ __attribute__((aligned(16))) char Vs[2 * SP * 64];
  __shared__ unsigned long long mk[2];

  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int qbase = blockIdx.y * SP;
  const int D = H * 64, ld = 3 * D;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const HT* base = qkv + (size_t)b * S * ld + h * 64;     // wave-uniform (blockIdx only)

  int nchunks = (S + SP - 1) / SP;
  if (causal) nchunks = min(nchunks, (qbase + SP - 1) / SP + 1);  // chunks entirely above the diagonal

  // this thread's pieces of a chunk: rows (tid + i*256) >> 3, 16-byte column c = tid & 7 (the same for every i)
  u32x4 kreg[NP], vreg[NP];
  auto fetch = [&](int kbase) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int row = (tid + i * 256) >> 3, c = tid & 7;
      const int rg = kbase + row < S ? kbase + row : S - 1;       // rows past the sequence end re-read the last row (masked)
      // wave-uniform base + 32-bit lane offset (a sample's qkv rows span < 4 GiB): scalar-base loads, no 64-bit lane arithmetic
      const unsigned off = ((unsigned)rg * (unsigned)ld + (unsigned)(c * 8)) * (unsigned)sizeof(HT);
      kreg[i] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(base + D) + off);
      vreg[i] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(base + 2 * D) + off);
    }
  };
  fetch(0);

  {  // the query block, whole 128-byte lines, GEMM swizzle: all four loads of a thread in flight together (rows past the
     // sequence end re-read its last row; their outputs are never stored)
    u32x4 q16[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int row = (tid + i * 256) >> 3, c = tid & 7;
      const int rg = qbase + row < S ? qbase + row : S - 1;
      q16[i] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(base) +
                                               ((unsigned)rg * (unsigned)ld + (unsigned)(c * 8)) * (unsigned)sizeof(HT));
    }
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int row = (tid + i * 256) >> 3, c = tid & 7;
      *reinterpret_cast<u32x4*>(k_image(Qs, row, c)) = q16[i];
    }
  }

  const int q0 = wave * 32;  // inside the block
  const bool active = qbase + q0 < S;
  const int lrow = lane & 31, hi = lane >> 5;
  const int qidx = qbase + q0 + lrow;
  const int lsw = (lrow >> 1) & 7;

  const char* vlane = Vs + vtr_lane_offset(lrow, hi);
  u32x4 qf[4];
  f32x16 acc[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[dt][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;  // l_run: this lane's half of the row sum

  for (int ch = 0; ch < nchunks; ++ch) {
    const int kbase = ch * SP;
    __syncthreads();  // everyone is done reading the previous chunk
    if (tid < SP) {
      const int key = kbase + tid;
      const bool ok = key < S && (key_mask == nullptr || key_mask[(size_t)b * S + key] != 0);
      const unsigned long long bits = __ballot(ok);
      if (lane == 0) mk[wave] = bits;
    }
#pragma unroll
    for (int i = 0; i < NP; ++i) {   // the chunk fetched during the previous iteration (or the prologue) -> LDS
      const int row = (tid + i * 256) >> 3, c = tid & 7;
      *reinterpret_cast<u32x4*>(k_image(Ks, row, c)) = kreg[i];
      *reinterpret_cast<u32x4*>(v_image(Vs, row, c, SP * 64)) = vreg[i];
    }
    if (ch + 1 < nchunks) fetch(kbase + SP);   // in flight while this chunk is multiplied
    __syncthreads();
    if (!active) continue;
    if (ch == 0) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) qf[ks] = image_fragment(Qs, q0 + lrow, ks, hi, lsw);
    }
    const unsigned long long mhalf[2] = {mk[0], mk[1]};
    constexpr int NKS = 4, NDT = 2, KPL = SP * 128, VIMG = SP * 64;   // one K plane: the term of KPL is 0
#include "attention_flash_step.inc"   // the online-softmax step over the chunk's two 64-key halves (3 waves/SIMD here)
  }
  if (!active) return;  // no workgroup barrier below
  {
    const float rsum = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = 1.0f / rsum;
    char* orow_lds = Qs + (q0 + lrow) * 128;  // this wave's own Q rows: consumed into qf long ago
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) stage_out4<HT, false>(orow_lds, lrow, hi, lsw, dt, q4, acc[dt], inv);   // this kernel stages without the odd-row exchange
    __builtin_amdgcn_wave_barrier();
    const int c = lane & 7;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int rl = q0 + it * 8 + (lane >> 3);
      const int r = qbase + rl;
      const u32x4 v = load_out_row<false>(Qs, rl, c);
      if (r < S) *reinterpret_cast<u32x4*>(out + ((size_t)b * S + r) * D + h * 64 + c * 8) = v;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Heads other than 64: 72 .. 128 columns, a multiple of 8 (ViT-H/14: 16 heads of 80, ViT-g/14: 16 of 88).  One kernel for every
// sequence length, modelled on attention_flash_kernel and taking the same online-softmax step: one workgroup = 128 queries of one
// (sample, head) (4 waves x 32), grid (B*H, ceil(S/128)), the keys streamed in 128-key chunks, causal option and key_mask.
//
// Head size: the kernel is instantiated for the PADDED size DP = 96 (head <= 96) or 128 and takes the head at run time.
//   * scores: DP/16 k-steps of v_mfma_f32_32x32x16.  The K image is DP/64 (rounded up: 2) planes of 64 columns, each the 128-byte
//     swizzled rows of attention_mfma_dev.h k_image, so a k-step reads plane ks >> 2 at step ks & 3 with the fragment read as it is.
//   * P V: DP/32 output tiles, one [keys][32] V image each (v_image / pv_step take the tile index as they are).
//   * a row has head/8 16-byte pieces in memory (h * head * 2 bytes is 16-byte aligned); the pieces head/8 .. DP/8 - 1 of the Q
//     fragments and of the K / V images are ZEROS, written and never read from memory (a head of 88 ends inside k-step 5: its
//     upper half is the zero piece).  They add exact zeros to the scores; their output columns are never stored.
//   * rows past the sequence end re-read row S - 1 (masked keys; queries that are never stored), as at head 64.
// What the head-64 kernel keeps in registers does not fit at DP = 128 (acc 64 + scores 32 + Q fragments 32 + 32 of prefetch
// staging): the register prefetch of the next chunk is gone -- a chunk's K rows, then its V rows, pass through 24 / 32 staging
// registers in front of the barrier -- and the Q fragments come straight from memory (as in the short-sequence kernel), so there is
// no Q image.  LDS: K 32 KB + V 24 / 32 KB = 56 / 64 KB, static -- the key validity words are two ballots of each wave's own, not
// LDS words, which keeps DP = 128 at 64 KB exactly: no dynamic LDS, no attribute.  Two workgroups per CU = two waves per SIMD, the
// occupancy the kernel is compiled for.  The normalised output tile is staged in the wave's own rows of the K planes once every
// wave is past the last chunk.
// Registers as hipcc reports them: profiles/head_dim_kernels.txt.
// ---------------------------------------------------------------------------------------------
namespace {

constexpr int kChunk = 128;                 // queries per workgroup, keys per chunk
constexpr int kPlane = kChunk * 128;        // one 64-column plane of the K image
constexpr int kVImage = kChunk * 64;        // one 32-column V image

template <typename HT, int DP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void attention_flash_hd_kernel(
    const HT* __restrict__ qkv, HT* __restrict__ out, int S, int H, int head, int causal, const int64_t* __restrict__ key_mask) {
  using X8 = typename half_traits<HT>::x8;
  static_assert(DP == 96 || DP == 128, "padded head sizes");
  constexpr int SP = kChunk;
  constexpr int NC = DP / 8;               // 16-byte pieces of a padded row
  constexpr int NKS = DP / 16;             // k-steps of the score product
  constexpr int NDT = DP / 32;             // 32-column output tiles
  constexpr int NP = SP * NC / 256;        // pieces of a chunk's K (or V) rows per thread: 6 / 8
  constexpr int KPL = kPlane, VIMG = kVImage;
  __shared__ __attribute__((aligned(16))) char Ks[2 * kPlane];        // 2 planes [SP][64 columns]
  __shared__ __attribute__((aligned(16))) char Vs[NDT * kVImage];    // NDT images [SP][32 columns]

  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int qbase = blockIdx.y * SP;
  const int D = H * head, ld = 3 * D;
  const int hc = head >> 3;                 // pieces of a row that exist
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const HT* base = qkv + (size_t)b * S * ld + h * head;     // wave-uniform (blockIdx only)

  int nchunks = (S + SP - 1) / SP;
  if (causal) nchunks = min(nchunks, (qbase + SP - 1) / SP + 1);  // chunks entirely above the diagonal

  const int q0 = wave * 32;  // inside the block
  const bool active = qbase + q0 < S;
  const int lrow = lane & 31, hi = lane >> 5;
  const int qidx = qbase + q0 + lrow;
  const int lsw = (lrow >> 1) & 7;
  const u32x4 zero16 = {0u, 0u, 0u, 0u};

  // Q fragments (B operand) straight from memory: Q[query = lrow][d = 16 ks + 8 hi .. + 7] = piece 2 ks + hi of the row; a piece
  // past the head is zero (the load goes to piece 0 instead: unconditional, and inside the row)
  u32x4 qf[NKS];
  {
    const unsigned qrow = (unsigned)(qidx < S ? qidx : S - 1) * (unsigned)ld;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      const int p = 2 * ks + hi;
      const u32x4 v = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(base) +
                                                      (qrow + (unsigned)((p < hc ? p : 0) * 8)) * (unsigned)sizeof(HT));
      qf[ks] = p < hc ? v : zero16;
    }
  }

  // one chunk's rows of K (which = 1) or V (which = 2) -> LDS: piece e = tid + 256 i is piece e % NC of row e / NC
  auto stage = [&](int kbase, int which) {
    u32x4 r[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int e = tid + i * 256, row = e / NC, c = e - row * NC;
      const int rg = kbase + row < S ? kbase + row : S - 1;       // rows past the sequence end re-read the last row (masked)
      // wave-uniform base + 32-bit lane offset (a sample's qkv rows span < 4 GiB): scalar-base loads, no 64-bit lane arithmetic
      const unsigned off = ((unsigned)rg * (unsigned)ld + (unsigned)((c < hc ? c : 0) * 8)) * (unsigned)sizeof(HT);
      const u32x4 v = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(base + which * D) + off);
      r[i] = c < hc ? v : zero16;
    }
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int e = tid + i * 256, row = e / NC, c = e - row * NC;
      if (which == 1) *reinterpret_cast<u32x4*>(k_image(Ks + (c >> 3) * kPlane, row, c & 7)) = r[i];
      else *reinterpret_cast<u32x4*>(v_image(Vs, row, c, kVImage)) = r[i];
    }
  };

  const char* vlane = Vs + vtr_lane_offset(lrow, hi);
  f32x16 acc[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[dt][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;  // l_run: this lane's half of the row sum

  for (int ch = 0; ch < nchunks; ++ch) {
    const int kbase = ch * SP;
    __syncthreads();  // everyone is done reading the previous chunk
    // key validity (sequence end and the tokenizer's attention_mask) of the chunk's two 64-key halves: every wave's own ballots
    unsigned long long mhalf[2];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const int key = kbase + 64 * hf + lane;
      mhalf[hf] = __ballot(key < S && (key_mask == nullptr || key_mask[(size_t)b * S + key] != 0));
    }
    stage(kbase, 1);
    stage(kbase, 2);
    __syncthreads();
    if (!active) continue;
#include "attention_flash_step.inc"   // the online-softmax step over the chunk's two 64-key halves
  }
  __syncthreads();  // every wave is past the last chunk: the K planes may now be reused as output staging
  if (!active) return;  // no workgroup barrier below
  {
    const float rsum = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = 1.0f / rsum;
    // the normalised 32 x DP tile into the wave's own rows of the K planes: output tile dt = columns 32 (dt & 1) .. of plane dt >> 1
    char* orow_lds = Ks + (q0 + lrow) * 128;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) stage_out4<HT, false>(orow_lds + (dt >> 1) * kPlane, lrow, hi, lsw, dt & 1, q4, acc[dt], inv);
    __builtin_amdgcn_wave_barrier();
    // the head's own pieces of the wave's 32 rows to memory, piece by piece along each row
#pragma unroll
    for (int it = 0; it < NC / 2; ++it) {
      const int e = lane + it * 64, rw = e / NC, c = e - rw * NC;
      const int rl = q0 + rw;
      const int r = qbase + rl;
      const u32x4 v = load_out_row<false>(Ks + (c >> 3) * kPlane, rl, c & 7);
      if (r < S && c < hc) *reinterpret_cast<u32x4*>(out + ((size_t)b * S + r) * D + h * head + c * 8) = v;
    }
  }
}

}  // namespace

// every sequence length of one operand type at DP = the head's instantiated size (dispatch.h with_pad)
template <typename HT, int DP>
static hipError_t launch_attention_mfma_t(const void* qkv, void* out, int B, int S, int H, int head, int causal,
                                          const int64_t* key_mask, hipStream_t s, const int* cu) {
  if constexpr (DP != 64) {   // the padded-head kernel: one for every S, no packed rows
    if (cu) return hipErrorInvalidValue;
    hipLaunchKernelGGL((attention_flash_hd_kernel<HT, DP>), dim3(B * H, (S + kChunk - 1) / kChunk), dim3(256), 0, s, (const HT*)qkv,
                       (HT*)out, S, H, head, causal, key_mask);
    return hipGetLastError();
  } else if (S > 128) {
    if (cu) return hipErrorInvalidValue;   // packed rows: short-sequence kernel only (captions are 77 tokens at most)
    hipLaunchKernelGGL(attention_flash_kernel<HT>, dim3(B * H, (S + 127) / 128), dim3(256), 0, s, (const HT*)qkv,
                       (HT*)out, S, H, causal, key_mask);
    return hipGetLastError();
  } else {
    const int KT = (S + 31) / 32;
    const dim3 grid(B * H), block(64 * KT);
#define PLIPMI_ATT(K) \
  hipLaunchKernelGGL((attention_mfma_kernel<HT, K>), grid, block, 0, s, (const HT*)qkv, (HT*)out, S, H, causal, key_mask, cu)
    switch (KT) {
      case 1: PLIPMI_ATT(1); break;
      case 2: PLIPMI_ATT(2); break;
      case 3: PLIPMI_ATT(3); break;
      default: PLIPMI_ATT(4); break;
    }
#undef PLIPMI_ATT
    return hipGetLastError();
  }
}

hipError_t launch_attention_mfma(const void* qkv, void* out, int dtype, int B, int S, int H, int head, int causal,
                                 const int64_t* key_mask, hipStream_t s, const int* cu) {
  if (S <= 0 || (dtype != 1 && dtype != 2) || !attention_head_ok(head)) return hipErrorInvalidValue;
  return with_half(dtype, [&](auto tag) {
    return with_pad(attention_head_pad(head), [&](auto pad) {
      return launch_attention_mfma_t<decltype(tag), decltype(pad)::value>(qkv, out, B, S, H, head, causal, key_mask, s, cu);
    });
  });
}

}  // namespace plipmi
