// attention_valu_hd.hip -- the exact-fp32 VALU attention kernel (attention.hip) for heads other than 64: 72 .. 128 columns, a
// multiple of 8 -- what the fp32 engine runs on a ViT-H/14 (heads of 80) or ViT-g/14 (88) vision tower, and the on-device checker
// of attention_mfma_hd.hip.  The kernel is the body of attention_valu_body.inc at a padded size DP = 96 (head <= 96) or 128, with 32
// keys per LDS tile (2 x 32 x DP x 4 bytes: 24 / 32 KB).  q and the accumulator are DP registers each: the 256-thread build keeps
// them in registers, the 1024-thread build (S > 256: 128 registers per lane) spills part of them to scratch -- exact, and slow;
// the 16-bit engines never take it.
#include "dispatch.h"
#include "kernels.h"

namespace plipmi {

constexpr int kKeyTileHd = 32;

template <typename T, int kMaxThreads, int DP>
__global__ __launch_bounds__(kMaxThreads) void attention_valu_hd_kernel(const T* __restrict__ qkv, T* __restrict__ out, int S, int H,
                                                                        int head, int causal, const int64_t* __restrict__ key_mask) {
  constexpr int KT = kKeyTileHd;
#include "attention_valu_body.inc"
}

hipError_t launch_attention_valu_hd(const void* qkv, void* out, int dtype, int B, int S, int H, int head, int causal,
                                    const int64_t* key_mask, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  if (S <= 0 || !attention_head_ok(head) || head == 64 || (dtype != 0 && dtype != 1 && dtype != 2)) return hipErrorInvalidValue;
  const int threads = ((S + 63) / 64) * 64;
  if (threads > 1024) return hipErrorInvalidValue;  // S <= 1024, as at head 64
  const dim3 grid(B * H), block(threads);
  with_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    with_pad(attention_head_pad(head), [&](auto pad) {
      constexpr int DP = decltype(pad)::value;
      if (threads <= 256)
        hipLaunchKernelGGL((attention_valu_hd_kernel<T, 256, DP>), grid, block, 0, s, (const T*)qkv, (T*)out, S, H, head, causal, key_mask);
      else
        hipLaunchKernelGGL((attention_valu_hd_kernel<T, 1024, DP>), grid, block, 0, s, (const T*)qkv, (T*)out, S, H, head, causal, key_mask);
    });
  });
  return hipGetLastError();
}

}  // namespace plipmi
