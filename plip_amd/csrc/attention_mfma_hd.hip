// attention_mfma_hd.hip -- MFMA attention of the two 16-bit engines for heads other than 64: 72 .. 128 columns, a multiple of 8
// (ViT-H/14: 16 heads of 80, ViT-g/14: 16 of 88).  One kernel for every sequence length, modelled on attention_mfma.hip's
// attention_flash_kernel and built from the same device pieces (attention_mfma_dev.h): one workgroup = 128 queries of one
// (sample, head) (4 waves x 32), grid (B*H, ceil(S/128)), the keys streamed in 128-key chunks with an online softmax, causal
// option and key_mask.  The products and their layouts -- scores^T = K Q^T, O^T = V^T P^T under the score accumulator's own key
// permutation, V^T through the transposing LDS read -- are those of attention_mfma.hip's header comment.
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
#include "attention_mfma_dev.h"
#include "dispatch.h"
#include "kernels.h"

namespace plipmi {

using namespace attn_dev;

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
    // two 64-key halves per staged chunk: 32 score registers live instead of 64, one online-softmax update per half
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      if (kbase + 64 * hf >= S) break;                           // wave-uniform: past the sequence end
      if (causal && kbase + 64 * hf > qbase + q0 + 31) break;  // wave-uniform: the rest is above the diagonal
      f32x16 sc[2];
      float cmax = -INFINITY;
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        const int t = 2 * hf + tt;
        const bool live = kbase + 32 * t < S && !(causal && kbase + 32 * t > qbase + q0 + 31);  // wave-uniform
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[tt][r] = 0.f;
        if (live) {
#pragma unroll
          for (int ks = 0; ks < NKS; ++ks)
            mma16<HT>(sc[tt], image_fragment(Ks + (ks >> 2) * kPlane, 32 * t + lrow, ks & 3, hi, lsw), qf[ks]);
        }
        unsigned bits = live ? (unsigned)(mhalf[hf] >> (32 * tt)) : 0u;   // the keys this lane may use: validity AND causal limit
        if (causal) bits &= causal_bits(qidx - (kbase + 32 * t));
        // every key of the tile usable by every query of the wave: no masking arithmetic at all
        if (__ballot(bits != 0xffffffffu) == 0ull) max_scores(sc[tt], cmax);
        else mask_scores(sc[tt], bits, hi, cmax);
      }
      cmax = fmaxf(cmax, __shfl_xor(cmax, 32, 64));
      const float m_new = fmaxf(m_run, cmax);
      const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
      const float m2 = m_use * kLog2e;
      const bool moved = m_new != m_run;    // (NaN-free: -inf != -inf is false, a first finite maximum is a move)
      // a lane whose maximum did not move rescales by EXACTLY 1 (attention_mfma.hip: l_run would drift against acc otherwise)
      const float scale = !moved ? 1.f : (m_run == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(fmaf(m_run, kLog2e, -m2));  // acc, l_run are 0 while m_run = -inf
      m_run = m_new;
      if (__ballot(moved) != 0ull) {        // wave-uniform: once the running maxima have settled the rescaling multiplies go
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[dt][r] *= scale;
      }
      float csum = 0.f;
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        const int t = 2 * hf + tt;
        if (kbase + 32 * t >= S || (causal && kbase + 32 * t > qbase + q0 + 31)) continue;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          X8 pf;
#pragma unroll
          for (int jj = 0; jj < 8; ++jj) {
            const float pv = __builtin_amdgcn_exp2f(fmaf(sc[tt][8 * s2 + jj], kLog2e, -m2));   // exp(x - m): one FMA + v_exp_f32
            csum += pv;
            pf[jj] = (HT)pv;
          }
#pragma unroll
          for (int dt = 0; dt < NDT; ++dt) acc[dt] = pv_step<HT>(vlane, kVImage, dt, 32 * t + 16 * s2, pf, acc[dt]);
        }
      }
      l_run = l_run * scale + csum;
    }
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

template <typename HT, int DP>
hipError_t launch_hd(const void* qkv, void* out, int B, int S, int H, int head, int causal, const int64_t* key_mask, hipStream_t s) {
  hipLaunchKernelGGL((attention_flash_hd_kernel<HT, DP>), dim3(B * H, (S + kChunk - 1) / kChunk), dim3(256), 0, s, (const HT*)qkv,
                     (HT*)out, S, H, head, causal, key_mask);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_attention_mfma_hd(const void* qkv, void* out, int dtype, int B, int S, int H, int head, int causal,
                                    const int64_t* key_mask, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  if (S <= 0 || (dtype != 1 && dtype != 2) || !attention_head_ok(head) || head == 64) return hipErrorInvalidValue;
  return with_half(dtype, [&](auto tag) {
    using HT = decltype(tag);
    return with_pad(attention_head_pad(head), [&](auto pad) {
      return launch_hd<HT, decltype(pad)::value>(qkv, out, B, S, H, head, causal, key_mask, s);
    });
  });
}

}  // namespace plipmi
