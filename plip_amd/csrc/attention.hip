// attention.hip -- softmax(Q K^T [+ causal / padding mask]) V per (image|caption, head)
// over the fused qkv activation (CLIPAttention.forward, modeling_clip.py:298-335 with
// eager_attention_forward :259-277; softmax statistics in fp32 like :271).
//
// head_dim is 64 for every OpenAI CLIP / PLIP variant (other heads, 72 .. 128: attention_valu_hd.hip and
// attention_mfma_hd.hip, dispatched from launch_attention below) and the sequences are tiny (50 vision
// tokens, 77 text tokens), so a whole (b, h) problem fits one workgroup:
//   * attention_valu_kernel  -- exact fp32 arithmetic (the fp32 engine's kernel, and the
//                               on-device checker for the MFMA kernel): one query row per
//                               lane, K/V tiles of 64 keys broadcast from LDS, flash-style
//                               online softmax in chunks of 8 keys.
//   * attention_mfma_kernel  -- bf16 MFMA kernel (attention_mfma.hip).
#include "dispatch.h"
#include "kernels.h"

namespace plipmi {

hipError_t launch_attention_mfma(const void* qkv, void* out, int dtype, int B, int S, int H, int causal, const int64_t* key_mask,
                                 hipStream_t s, const int* cu);

constexpr int kDh = 64;      // head dim of the kernels in this unit and in attention_mfma.hip
constexpr int kKeyTile = 64;  // keys staged in LDS per step

template <typename T, int kMaxThreads>
__global__ __launch_bounds__(kMaxThreads) void attention_valu_kernel(const T* __restrict__ qkv, T* __restrict__ out, int S,
                                                              int H, int causal, const int64_t* __restrict__ key_mask) {
  constexpr int DP = kDh, KT = kKeyTile, head = kDh;
#include "attention_valu_body.inc"   // the body, shared with the other head sizes (attention_valu_hd.hip)
}

hipError_t launch_attention(const void* qkv, void* out, int dtype, int B, int S, int H, int head, int causal,
                            const int64_t* key_mask, int impl, hipStream_t s, const int* cu) {
  if (B <= 0) return hipSuccess;
  if (!attention_head_ok(head)) return hipErrorInvalidValue;
  if (head != kDh) {   // the padded-head kernels: one MFMA kernel for every S, no packed rows
    if (cu || S <= 0) return hipErrorInvalidValue;
    if (impl == 1) return launch_attention_mfma_hd(qkv, out, dtype, B, S, H, head, causal, key_mask, s);
    return launch_attention_valu_hd(qkv, out, dtype, B, S, H, head, causal, key_mask, s);
  }
  if (impl == 1) {
    if (dtype != 1 && dtype != 2) return hipErrorInvalidValue;
    return launch_attention_mfma(qkv, out, dtype, B, S, H, causal, key_mask, s, cu);
  }
  if (cu) return hipErrorInvalidValue;   // packed rows are an MFMA-kernel form
  const int threads = ((S + 63) / 64) * 64;
  if (threads > 1024) return hipErrorInvalidValue;  // S <= 1024 (ViT-L/14@336 has 577 tokens)
  const dim3 grid(B * H), block(threads);
  // <= 256 threads: the register allocator may use 256 VGPRs (q[64] + acc[64] live); the 1024-thread
  // build (S > 256, e.g. ViT-L/14@336) trades some spills for the larger block.
  with_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    if (threads <= 256) hipLaunchKernelGGL((attention_valu_kernel<T, 256>), grid, block, 0, s, (const T*)qkv, (T*)out, S, H, causal, key_mask);
    else hipLaunchKernelGGL((attention_valu_kernel<T, 1024>), grid, block, 0, s, (const T*)qkv, (T*)out, S, H, causal, key_mask);
  });
  return hipGetLastError();
}

}  // namespace plipmi
