// attention_probs.hip -- the attention probabilities P[b, h, i, j] of HF's eager attention (CLIPAttention with
// output_attentions=True, modeling_clip.py eager_attention_forward: softmax(q k^T + causal + padding mask) in fp32),
// read from the fused qkv activation the q/k/v GEMM writes ([B*S, 3D]: q | k | v, head h at columns head h .. head h + head - 1).
// The score scale head^-1/2 is already folded into q (engine.hip pack_tower), so the kernel does not apply it.  Heads of
// 72 .. 128 run the same body at a padded size: every dot product runs over the head's own columns in ascending order, the arithmetic
// of the head-64 kernel with another trip count, hence the same bit-for-bit agreement with the summaries (attention_summary.hip).
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
  probs_block<T, kDh>(qkv, probs, S, H, kDh, causal, key_mask);   // attention_probs_dev.h: the body, shared with the other head sizes
}

// heads of 72 .. 128: the body at a padded size DP = 96 (head <= 96) or 128, the head a run-time argument
template <typename T, int DP>
__global__ __launch_bounds__(kThreads) void attention_probs_hd_kernel(const T* __restrict__ qkv, float* __restrict__ probs, int S, int H,
                                                                      int head, int causal, const int64_t* __restrict__ key_mask) {
  probs_block<T, DP>(qkv, probs, S, H, head, causal, key_mask);
}

}  // namespace

hipError_t launch_attention_probs(const void* qkv, float* probs, int dtype, int B, int S, int H, int head, int causal,
                                  const int64_t* key_mask, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  if (S <= 0 || S > 1024 || H <= 0 || !qkv || !probs || !attention_head_ok(head)) return hipErrorInvalidValue;
  if (dtype != 0 && dtype != 1 && dtype != 2) return hipErrorInvalidValue;
  const dim3 grid((S + kRows - 1) / kRows, H, B);
  return with_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return with_pad(attention_head_pad(head), [&](auto pad) {
      constexpr int DP = decltype(pad)::value;
      const size_t lds = probs_lds_bytes(S, DP);    // <= 16 x 1088 x 4 = 68 KiB at head 64 (S = 1024)
      if constexpr (DP == kDh) return launch_with_lds(&attention_probs_kernel<T>, grid, lds, s, qkv, probs, S, H, causal, key_mask);
      else return launch_with_lds(&attention_probs_hd_kernel<T, DP>, grid, lds, s, qkv, probs, S, H, head, causal, key_mask);
    });
  });
}

}  // namespace plipmi
