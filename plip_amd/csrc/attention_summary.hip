// attention_summary.hip -- the two summaries of the attention probabilities that plipmi_encode_attention_summary hands out without
// ever forming P [B, H, S, S] (include/plipmi.h): the pooled query row of every (block, head), and attention rollout (Abnar &
// Zuidema 2020, residual weight 1/2, head mean).  Both read the fused qkv activation of the block's q/k/v GEMM, as attention_probs.hip
// does, and are built from its two phases (attention_probs_dev.h): a probability they use is the bits attention_probs_kernel writes.
//
//   attention_pooled_rows   one workgroup per (b, h): the score row of query rows[b] against every key (a 1-row tile), its softmax
//                           by wave 0, stored to out [B, H, S].
//   attention_rollout_step  one workgroup per (b, tile of 16 query rows): for h = 0 .. H-1 the 16 x S probability tile is formed in
//                           LDS and added into an LDS tile A [16][S] (so the head sum runs in the order h = 0 .. H-1); then
//                           A^ = (1/2H) A + 1/2 I and R_out[b][tile rows] = A^ . R_in[b], fp32, k = 0 .. S-1 ascending in one fmaf
//                           chain per output.  R_in is read from memory (lanes own output columns: coalesced rows of R_in), A^ is
//                           broadcast from LDS four k at a time.  Every tile reads all of R_in[b], so R_out must be another buffer.
//                           R_in == nullptr is the identity: the tile of A^ is stored as it is (the bits the product with an explicit
//                           identity gives -- the other terms are exact zeros).
//                           LDS: 16 x (64 + S + S4) x 4 bytes, S4 = S rounded up to 4 -- 135 KB at S = 1024 (head 64; 139 KB at a
//                           padded head of 128).
//                           With row_idx / pooled_out it also stores the pooled query row of every head on its way (the tile that
//                           holds row rows[b] forms it anyway): the walk then needs no attention_pooled_rows launch.
//   attention_rollout_row   out [B, S] = row rows[b] of R [B, S, S].
// Heads of 72 .. 128 run the same bodies at a padded size (the _hd kernels below).
// All stores are ordinary vector stores; nothing here uses inline assembly.
#include "dispatch.h"
#include "attention_probs_dev.h"

namespace plipmi {

namespace {

using namespace probs_dev;

template <typename T>
__global__ __launch_bounds__(kThreads) void attention_pooled_rows_kernel(const T* __restrict__ qkv, const int* __restrict__ row_idx,
                                                                         float* __restrict__ out, int S, int H, int causal,
                                                                         const int64_t* __restrict__ key_mask) {
  pooled_rows_block<T, kDh>(qkv, row_idx, out, S, H, kDh, causal, key_mask);   // attention_probs_dev.h: the bodies, shared with the other head sizes
}

// RPL: tile rows per lane in the score phase and in the product (attention_probs_dev.h score_tile): 16 for long sequences, fewer
// where S is below the workgroup's 256 lanes, so that all four waves work
template <typename T, int RPL>
__global__ __launch_bounds__(kThreads) void attention_rollout_step_kernel(const T* __restrict__ qkv, const float* __restrict__ R_in,
                                                                          float* __restrict__ R_out, int S, int H, int causal,
                                                                          const int64_t* __restrict__ key_mask,
                                                                          const int* __restrict__ row_idx, float* __restrict__ pooled_out) {
  constexpr int DP = kDh, head = kDh;
#include "attention_rollout_body.inc"
}

// heads of 72 .. 128: the two bodies at a padded size DP = 96 (head <= 96) or 128, the head a run-time argument
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

__global__ __launch_bounds__(256) void attention_rollout_row_kernel(const float* __restrict__ R, const int* __restrict__ row_idx,
                                                                    float* __restrict__ out, int S) {
  const int b = blockIdx.x;
  const int r = min(max(row_idx[b], 0), S - 1);
  const float* src = R + ((size_t)b * S + r) * S;
  for (int j = threadIdx.x; j < S; j += 256) out[(size_t)b * S + j] = src[j];
}

template <typename T, int RPL, int DP>
hipError_t rollout_step_rpl(const void* qkv, const float* R_in, float* R_out, int B, int S, int H, int head, int causal,
                            const int64_t* key_mask, const int* rows, float* pooled_out, hipStream_t s) {
  const size_t lds = rollout_lds_bytes(S, DP);
  const dim3 grid((S + kRows - 1) / kRows, B);
  if constexpr (DP == kDh)
    return launch_with_lds(&attention_rollout_step_kernel<T, RPL>, grid, lds, s, qkv, R_in, R_out, S, H, causal, key_mask, rows, pooled_out);
  else
    return launch_with_lds(&attention_rollout_step_hd_kernel<T, RPL, DP>, grid, lds, s, qkv, R_in, R_out, S, H, head, causal, key_mask, rows,
                           pooled_out);
}

}  // namespace

size_t attention_rollout_lds_bytes(int S, int head) { return rollout_lds_bytes(S, attention_head_pad(head)); }

hipError_t launch_attention_pooled_rows(const void* qkv, const int* rows, float* out, int dtype, int B, int S, int H, int head, int causal,
                                        const int64_t* key_mask, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  if (S <= 0 || S > 1024 || H <= 0 || B > 65535 || !qkv || !rows || !out || !attention_head_ok(head)) return hipErrorInvalidValue;
  if (dtype != 0 && dtype != 1 && dtype != 2) return hipErrorInvalidValue;
  return with_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return with_pad(attention_head_pad(head), [&](auto pad) {
      constexpr int DP = decltype(pad)::value;
      const size_t lds = pooled_rows_lds_bytes(S, DP);
      if constexpr (DP == kDh) return launch_with_lds(&attention_pooled_rows_kernel<T>, dim3(H, B), lds, s, qkv, rows, out, S, H, causal, key_mask);
      else return launch_with_lds(&attention_pooled_rows_hd_kernel<T, DP>, dim3(H, B), lds, s, qkv, rows, out, S, H, head, causal, key_mask);
    });
  });
}

hipError_t launch_attention_rollout_step(const void* qkv, const float* R_in, float* R_out, int dtype, int B, int S, int H, int head,
                                         int causal, const int64_t* key_mask, hipStream_t s, const int* rows, float* pooled_out) {
  if (B <= 0) return hipSuccess;
  if (S <= 0 || S > 1024 || H <= 0 || B > 65535 || !qkv || !R_out || R_in == R_out || (pooled_out && !rows) || !attention_head_ok(head))
    return hipErrorInvalidValue;
  if (dtype != 0 && dtype != 1 && dtype != 2) return hipErrorInvalidValue;
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

hipError_t launch_attention_rollout_row(const float* R, const int* rows, float* out, int B, int S, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  if (S <= 0 || !R || !rows || !out) return hipErrorInvalidValue;
  hipLaunchKernelGGL(attention_rollout_row_kernel, dim3(B), dim3(256), 0, s, R, rows, out, S);
  return hipGetLastError();
}

}  // namespace plipmi
