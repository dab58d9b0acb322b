// attention_probs.hip -- the attention probabilities P[b, h, i, j] of HF's eager attention (CLIPAttention with
// output_attentions=True, modeling_clip.py eager_attention_forward: softmax(q k^T + causal + padding mask) in fp32),
// read from the fused qkv activation the q/k/v GEMM writes ([B*S, 3D]: q | k | v, head h at columns 64 h .. 64 h + 63).
// The score scale 64^-1/2 is already folded into q (engine.hip pack_tower), so the kernel does not apply it.
//
// Only plipmi_encode_tower_outputs launches it: the encode paths never form P (attention_mfma.hip keeps an online softmax,
// qkv_attention.hip never writes qkv).  It is write-bound -- fp32 [B, H, S, S] per layer, 30.7 MB for ViT-B/32 vision at
// B = 256 against 0.98 GFLOP of scores -- so the scores run on the VALU in fp32 and the work goes into the stores:
//   * one workgroup per (b, h, block of kRows query rows); the block's q rows are staged in LDS as fp32;
//   * phase 1: one key per lane (k row read as 16-byte loads, converted to fp32), kRows dot products against the
//     LDS-broadcast q rows, scores into an LDS tile [kRows][S] (masked entries -inf; under the causal mask the keys past
//     the block's last row are not computed);
//   * phase 2: one wave per row: max and sum by wave reductions, then p = exp(s - max) / sum stored lane-contiguous
//     (each wave store covers 256 contiguous bytes of the row).
// Masking follows HF: causal (text), key padding from the attention mask (text), none for vision.  Every masked entry is
// exp(-inf) = exactly 0.0; a row with no live key at all (HF: NaN) is written as zeros.
#include "dispatch.h"
#include "attention_probs_dev.h"

namespace plipmi {

namespace {

using namespace probs_dev;   // kDh, kRows, kThreads and the two phases (shared with attention_summary.hip)

template <typename T>
__global__ __launch_bounds__(kThreads) void attention_probs_kernel(const T* __restrict__ qkv, float* __restrict__ probs, int S, int H,
                                                                   int causal, const int64_t* __restrict__ key_mask) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* qs = lds;                    // [kRows][kDh]
  float* sc = lds + kRows * kDh;      // [kRows][S]

  const int i0 = blockIdx.x * kRows, h = blockIdx.y, b = blockIdx.z;
  const int D = H * kDh, ld = 3 * D;
  const int tid = threadIdx.x;
  const int rows = min(kRows, S - i0);
  const T* base = qkv + (size_t)b * S * ld + h * kDh;

  // q rows of the block -> LDS (rows past S: zeros, never stored)
  stage_q<T, kRows>(qs, base, ld, i0, rows, tid);
  __syncthreads();

  // phase 1: scores of every (row, key) of the block, one key per lane
  score_tile<T, kRows, kRows>(qs, sc, base, ld, D, S, i0, rows, b, causal, key_mask, tid);
  __syncthreads();

  // phase 2: one wave per row -- softmax statistics, then the normalised row
  const int lane = tid & 63, wave = tid >> 6;
  for (int r = wave; r < rows; r += kThreads / 64) {
    float* pr = probs + (((size_t)b * H + h) * S + (i0 + r)) * S;
    softmax_row(sc + r * S, S, lane, [pr](int j, float p) { pr[j] = p; });
  }
}

size_t attention_probs_lds_bytes(int S) { return (size_t)kRows * (kDh + S) * sizeof(float); }

}  // namespace

hipError_t launch_attention_probs(const void* qkv, float* probs, int dtype, int B, int S, int H, int causal, const int64_t* key_mask,
                                  hipStream_t s) {
  if (B <= 0) return hipSuccess;
  if (S <= 0 || S > 1024 || H <= 0 || !qkv || !probs) return hipErrorInvalidValue;
  const size_t lds = attention_probs_lds_bytes(S);    // <= 16 x 1088 x 4 = 68 KiB (S = 1024)
  const dim3 grid((S + kRows - 1) / kRows, H, B), block(kThreads);
  if (dtype != 0 && dtype != 1 && dtype != 2) return hipErrorInvalidValue;
  return with_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    if (lds > 64 * 1024) {
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&attention_probs_kernel<T>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(attention_probs_kernel<T>, grid, block, lds, s, (const T*)qkv, probs, S, H, causal, key_mask);
    return hipGetLastError();
  });
}

}  // namespace plipmi
