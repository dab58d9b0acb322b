// attention.hip -- softmax(Q K^T [+ causal / padding mask]) V per (image|caption, head)
// over the fused qkv activation (CLIPAttention.forward, modeling_clip.py:298-335 with
// eager_attention_forward :259-277; softmax statistics in fp32 like :271).
//
// head_dim is 64 for every OpenAI CLIP / PLIP variant (other heads, 72 .. 128: the same kernels at a padded
// size, dispatched from launch_attention below) and the sequences are tiny (50 vision
// tokens, 77 text tokens), so a whole (b, h) problem fits one workgroup:
//   * attention_valu_kernel  -- exact fp32 arithmetic (the fp32 engine's kernel, and the
//                               on-device checker for the MFMA kernel): one query row per
//                               lane, K/V tiles of 64 keys broadcast from LDS, flash-style
//                               online softmax in chunks of 8 keys.
//   * attention_mfma_kernel  -- bf16 MFMA kernel (attention_mfma.hip).
#include "dispatch.h"
#include "kernels.h"

namespace plipmi {

// attention_mfma.hip: the MFMA kernels of every head size (dtype bf16 or f16; cu: head 64, S <= 128)
hipError_t launch_attention_mfma(const void* qkv, void* out, int dtype, int B, int S, int H, int head, int causal,
                                 const int64_t* key_mask, hipStream_t s, const int* cu);

constexpr int kDh = 64;      // head dim of the OpenAI CLIP / PLIP variants
// keys staged in LDS per step at DP columns per lane (2 x KT x DP x 4 bytes of LDS: 32 KB at 64, 24 / 32 KB at 96 / 128)
constexpr int key_tile(int DP) { return DP == kDh ? 64 : 32; }

template <typename T, int kMaxThreads>
__global__ __launch_bounds__(kMaxThreads) void attention_valu_kernel(const T* __restrict__ qkv, T* __restrict__ out, int S,
                                                              int H, int causal, const int64_t* __restrict__ key_mask) {
  constexpr int DP = kDh, KT = key_tile(DP), head = kDh;
#include "attention_valu_body.inc"
}

// Heads other than 64 (72 .. 128 columns, a multiple of 8 -- what the fp32 engine runs on a ViT-H/14 (heads of 80) or ViT-g/14 (88)
// vision tower, and the on-device checker of the padded MFMA kernel): the same body at a padded size DP = 96 (head <= 96) or 128,
// the head a run-time argument.  q and the accumulator are DP registers each: the 256-thread build keeps them in registers, the
// 1024-thread build (S > 256: 128 registers per lane) spills part of them to scratch -- exact, and slow; the 16-bit engines never take it.
template <typename T, int kMaxThreads, int DP>
__global__ __launch_bounds__(kMaxThreads) void attention_valu_hd_kernel(const T* __restrict__ qkv, T* __restrict__ out, int S, int H,
                                                                        int head, int causal, const int64_t* __restrict__ key_mask) {
  constexpr int KT = key_tile(DP);
#include "attention_valu_body.inc"
}

template <typename T, int kMaxThreads, int DP>
static void launch_valu(dim3 grid, dim3 block, hipStream_t s, const void* qkv, void* out, int S, int H, int head, int causal,
                        const int64_t* key_mask) {
  if constexpr (DP == kDh)
    hipLaunchKernelGGL((attention_valu_kernel<T, kMaxThreads>), grid, block, 0, s, (const T*)qkv, (T*)out, S, H, causal, key_mask);
  else
    hipLaunchKernelGGL((attention_valu_hd_kernel<T, kMaxThreads, DP>), grid, block, 0, s, (const T*)qkv, (T*)out, S, H, head, causal, key_mask);
}

hipError_t launch_attention(const void* qkv, void* out, int dtype, int B, int S, int H, int head, int causal,
                            const int64_t* key_mask, int impl, hipStream_t s, const int* cu) {
  if (B <= 0) return hipSuccess;
  if (S <= 0 || !attention_head_ok(head) || (dtype != 0 && dtype != 1 && dtype != 2)) return hipErrorInvalidValue;
  if (impl == 1) return launch_attention_mfma(qkv, out, dtype, B, S, H, head, causal, key_mask, s, cu);
  if (cu) return hipErrorInvalidValue;   // packed rows are an MFMA-kernel form
  const int threads = ((S + 63) / 64) * 64;
  if (threads > 1024) return hipErrorInvalidValue;  // S <= 1024 (ViT-L/14@336 has 577 tokens)
  const dim3 grid(B * H), block(threads);
  // <= 256 threads: the register allocator may use 256 VGPRs (q[DP] + acc[DP] live); the 1024-thread
  // build (S > 256, e.g. ViT-L/14@336) trades some spills for the larger block.
  with_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    with_pad(attention_head_pad(head), [&](auto pad) {
      constexpr int DP = decltype(pad)::value;
      if (threads <= 256) launch_valu<T, 256, DP>(grid, block, s, qkv, out, S, H, head, causal, key_mask);
      else launch_valu<T, 1024, DP>(grid, block, s, qkv, out, S, H, head, causal, key_mask);
    });
  });
  return hipGetLastError();
}

}  // namespace plipmi
