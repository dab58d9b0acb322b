// attention_probs.hip -- the attention probabilities P[b, h, i, j] of HF's eager attention (CLIPAttention with
// output_attentions=True, modeling_clip.py eager_attention_forward: softmax(q k^T + causal + padding mask) in fp32),
// read from the fused qkv activation the q/k/v GEMM writes ([B*S, 3D]: q | k | v, head h at columns head h .. head h + head - 1).
// The score scale head^-1/2 is already folded into q (engine.hip pack_tower), so the kernel does not apply it.  This unit holds
// the head-64 kernel; heads of 72 .. 128 run the same body at a padded size from attention_probs_hd.hip.
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

}  // namespace

hipError_t launch_attention_probs(const void* qkv, float* probs, int dtype, int B, int S, int H, int head, int causal,
                                  const int64_t* key_mask, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  if (S <= 0 || S > 1024 || H <= 0 || !qkv || !probs || !attention_head_ok(head)) return hipErrorInvalidValue;
  if (head != kDh) return launch_attention_probs_hd(qkv, probs, dtype, B, S, H, head, causal, key_mask, s);
  const size_t lds = probs_lds_bytes(S, kDh);    // <= 16 x 1088 x 4 = 68 KiB (S = 1024)
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
