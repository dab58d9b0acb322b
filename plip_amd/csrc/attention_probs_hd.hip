// attention_probs_hd.hip -- the attention probabilities and their two summaries (attention_probs.hip, attention_summary.hip) for
// heads other than 64: 72 .. 128 columns, a multiple of 8 (the ViT-H/14 vision tower has 16 heads of 80, ViT-g/14 16 of 88).
// The kernels are the bodies of attention_probs_dev.h / attention_rollout_body.inc at a padded size DP = 96 (head <= 96) or 128: a q row has DP columns in
// LDS, those past the head are zeros, and every dot product runs over the head's own columns in ascending order -- the
// arithmetic of the head-64 kernels with another trip count, hence the same bit-for-bit agreement between the probabilities,
// the pooled rows and the rows a rollout step stores.  Grids, the phases and the LDS layout: the units named above.
#include "dispatch.h"
#include "attention_probs_dev.h"

namespace plipmi {

namespace {

using namespace probs_dev;

template <typename T, int DP>
__global__ __launch_bounds__(kThreads) void attention_probs_hd_kernel(const T* __restrict__ qkv, float* __restrict__ probs, int S, int H,
                                                                      int head, int causal, const int64_t* __restrict__ key_mask) {
  probs_block<T, DP>(qkv, probs, S, H, head, causal, key_mask);
}

template <typename T, int DP>
__global__ __launch_bounds__(kThreads) void attention_pooled_rows_hd_kernel(const T* __restrict__ qkv, const int* __restrict__ row_idx,
                                                                            float* __restrict__ out, int S, int H, int head, int causal,
                                                                            const int64_t* __restrict__ key_mask) {
  pooled_rows_block<T, DP>(qkv, row_idx, out, S, H, head, causal, key_mask);
}

template <typename T, int RPL, int DP>
__global__ __launch_bounds__(kThreads) void attention_rollout_step_hd_kernel(const T* __restrict__ qkv, const float* __restrict__ R_in,
                                                                             float* __restrict__ R_out, int S, int H, int head, int causal,
                                                                             const int64_t* __restrict__ key_mask,
                                                                             const int* __restrict__ row_idx,
                                                                             float* __restrict__ pooled_out) {
#include "attention_rollout_body.inc"
}

template <typename T, int RPL, int DP>
hipError_t rollout_step_rpl(const void* qkv, const float* R_in, float* R_out, int B, int S, int H, int head, int causal,
                            const int64_t* key_mask, const int* rows, float* pooled_out, hipStream_t s) {
  const size_t lds = rollout_lds_bytes(S, DP);
  const hipError_t e = allow_lds(&attention_rollout_step_hd_kernel<T, RPL, DP>, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((attention_rollout_step_hd_kernel<T, RPL, DP>), dim3((S + kRows - 1) / kRows, B), dim3(kThreads), lds, s,
                     (const T*)qkv, R_in, R_out, S, H, head, causal, key_mask, rows, pooled_out);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_attention_probs_hd(const void* qkv, float* probs, int dtype, int B, int S, int H, int head, int causal,
                                     const int64_t* key_mask, hipStream_t s) {
  const dim3 grid((S + kRows - 1) / kRows, H, B), block(kThreads);
  return with_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return with_pad(attention_head_pad(head), [&](auto pad) {
      constexpr int DP = decltype(pad)::value;
      const size_t lds = probs_lds_bytes(S, DP);
      const hipError_t e = allow_lds(&attention_probs_hd_kernel<T, DP>, lds);
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL((attention_probs_hd_kernel<T, DP>), grid, block, lds, s, (const T*)qkv, probs, S, H, head, causal, key_mask);
      return hipGetLastError();
    });
  });
}

hipError_t launch_attention_pooled_rows_hd(const void* qkv, const int* rows, float* out, int dtype, int B, int S, int H, int head,
                                           int causal, const int64_t* key_mask, hipStream_t s) {
  return with_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return with_pad(attention_head_pad(head), [&](auto pad) {
      constexpr int DP = decltype(pad)::value;
      hipLaunchKernelGGL((attention_pooled_rows_hd_kernel<T, DP>), dim3(H, B), dim3(kThreads), pooled_rows_lds_bytes(S, DP), s,
                         (const T*)qkv, rows, out, S, H, head, causal, key_mask);
      return hipGetLastError();
    });
  });
}

hipError_t launch_attention_rollout_step_hd(const void* qkv, const float* R_in, float* R_out, int dtype, int B, int S, int H, int head,
                                            int causal, const int64_t* key_mask, hipStream_t s, const int* rows, float* pooled_out) {
  return with_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return with_pad(attention_head_pad(head), [&](auto pad) {
      constexpr int DP = decltype(pad)::value;
      if (S <= 64) return rollout_step_rpl<T, 4, DP>(qkv, R_in, R_out, B, S, H, head, causal, key_mask, rows, pooled_out, s);
      if (S <= 128) return rollout_step_rpl<T, 8, DP>(qkv, R_in, R_out, B, S, H, head, causal, key_mask, rows, pooled_out, s);
      return rollout_step_rpl<T, 16, DP>(qkv, R_in, R_out, B, S, H, head, causal, key_mask, rows, pooled_out, s);
    });
  });
}

}  // namespace plipmi
