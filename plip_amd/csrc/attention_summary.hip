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
//                           LDS: 16 x (64 + S + S4) x 4 bytes, S4 = S rounded up to 4 -- 135 KB at S = 1024.
//                           With row_idx / pooled_out it also stores the pooled query row of every head on its way (the tile that
//                           holds row rows[b] forms it anyway): the walk then needs no attention_pooled_rows launch.
//   attention_rollout_row   out [B, S] = row rows[b] of R [B, S, S].
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
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* qs = lds;            // [1][kDh]
  float* sc = lds + kDh;      // [1][S]
  const int h = blockIdx.x, b = blockIdx.y;
  const int D = H * kDh, ld = 3 * D;
  const int tid = threadIdx.x;
  const int i0 = min(max(row_idx[b], 0), S - 1);    // (the pooling rule only yields rows of the sequence; a caller's array is clamped)
  const T* base = qkv + (size_t)b * S * ld + h * kDh;
  stage_q<T, 1>(qs, base, ld, i0, 1, tid);
  __syncthreads();
  score_tile<T, 1, 1>(qs, sc, base, ld, D, S, i0, 1, b, causal, key_mask, tid);
  __syncthreads();
  if (tid < 64) {
    float* pr = out + ((size_t)b * H + h) * S;
    softmax_row(sc, S, tid, [pr](int j, float p) { pr[j] = p; });
  }
}

// RPL: tile rows per lane in the score phase and in the product (attention_probs_dev.h score_tile): 16 for long sequences, fewer
// where S is below the workgroup's 256 lanes, so that all four waves work
template <typename T, int RPL>
__global__ __launch_bounds__(kThreads) void attention_rollout_step_kernel(const T* __restrict__ qkv, const float* __restrict__ R_in,
                                                                          float* __restrict__ R_out, int S, int H, int causal,
                                                                          const int64_t* __restrict__ key_mask,
                                                                          const int* __restrict__ row_idx, float* __restrict__ pooled_out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int S4 = (S + 3) & ~3;
  float* qs = lds;                       // [kRows][kDh]
  float* ab = qs + kRows * kDh;          // [kRows][S4]: the head sum, then A^ (columns S .. S4: zeros)
  float* sc = ab + kRows * S4;           // [kRows][S]
  const int i0 = blockIdx.x * kRows, b = blockIdx.y;
  const int D = H * kDh, ld = 3 * D;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int rows = min(kRows, S - i0);
  // the tile that holds the pooled row also stores P[b, h][pooled row, :] (fp32 [B, H, S]): pooled_r = its tile row there, else -1
  const int pooled_r = pooled_out ? min(max(row_idx[b], 0), S - 1) - i0 : -1;
  float* pooled_b = (pooled_r >= 0 && pooled_r < kRows) ? pooled_out + (size_t)b * H * S : nullptr;

  for (int e = tid; e < kRows * S4; e += kThreads) ab[e] = 0.f;
  for (int h = 0; h < H; ++h) {
    const T* base = qkv + (size_t)b * S * ld + h * kDh;
    stage_q<T, kRows>(qs, base, ld, i0, rows, tid);
    __syncthreads();
    score_tile<T, kRows, RPL>(qs, sc, base, ld, D, S, i0, rows, b, causal, key_mask, tid);
    __syncthreads();
    for (int r = wave; r < rows; r += kThreads / 64) {     // row r is wave r % 4's in every head: no two waves touch one row of ab
      float* ar = ab + r * S4;
      float* pr = (pooled_b && r == pooled_r) ? pooled_b + (size_t)h * S : nullptr;
      softmax_row_in_place(sc + r * S, S, lane, [ar, pr](int j, float p) {
#pragma clang fp contract(off)      // the sum of the probabilities as stored: p is rounded before it is added
        ar[j] = ar[j] + p;
        if (pr) pr[j] = p;
      });
    }
    __syncthreads();
  }

  // A^ = (1/2) (A / H) + (1/2) I
  const float half_mean = 0.5f / (float)H;
  for (int e = tid; e < kRows * S4; e += kThreads) {
    const int r = e / S4, k = e - r * S4;
    const float a = ab[e] * half_mean;
    ab[e] = (r < rows && k == i0 + r) ? a + 0.5f : a;
  }
  __syncthreads();

  constexpr int kLanes = kThreads / (kRows / RPL);
  const int r0 = (tid / kLanes) * RPL;
  float* out = R_out + ((size_t)b * S + i0) * S;
  if (R_in == nullptr) {
    for (int c = tid % kLanes; c < S; c += kLanes)
#pragma unroll
      for (int r = 0; r < RPL; ++r)
        if (r0 + r < rows) out[(size_t)(r0 + r) * S + c] = ab[(r0 + r) * S4 + c];
    return;
  }
  const float* Rb = R_in + (size_t)b * S * S;
  for (int c = tid % kLanes; c < S; c += kLanes) {
    float acc[RPL];
#pragma unroll
    for (int r = 0; r < RPL; ++r) acc[r] = 0.f;
    int k = 0;
    for (; k + 3 < S; k += 4) {
      const float x0 = Rb[(size_t)k * S + c], x1 = Rb[(size_t)(k + 1) * S + c], x2 = Rb[(size_t)(k + 2) * S + c],
                  x3 = Rb[(size_t)(k + 3) * S + c];
#pragma unroll
      for (int r = 0; r < RPL; ++r) {
        const float4 a = *reinterpret_cast<const float4*>(&ab[(r0 + r) * S4 + k]);
        acc[r] = fmaf(a.x, x0, acc[r]);
        acc[r] = fmaf(a.y, x1, acc[r]);
        acc[r] = fmaf(a.z, x2, acc[r]);
        acc[r] = fmaf(a.w, x3, acc[r]);
      }
    }
    for (; k < S; ++k) {
      const float x = Rb[(size_t)k * S + c];
#pragma unroll
      for (int r = 0; r < RPL; ++r) acc[r] = fmaf(ab[(r0 + r) * S4 + k], x, acc[r]);
    }
#pragma unroll
    for (int r = 0; r < RPL; ++r)
      if (r0 + r < rows) out[(size_t)(r0 + r) * S + c] = acc[r];
  }
}

__global__ __launch_bounds__(256) void attention_rollout_row_kernel(const float* __restrict__ R, const int* __restrict__ row_idx,
                                                                    float* __restrict__ out, int S) {
  const int b = blockIdx.x;
  const int r = min(max(row_idx[b], 0), S - 1);
  const float* src = R + ((size_t)b * S + r) * S;
  for (int j = threadIdx.x; j < S; j += 256) out[(size_t)b * S + j] = src[j];
}

template <typename K>
hipError_t allow_lds(K kernel, size_t lds) {
  if (lds <= 64 * 1024) return hipSuccess;
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

template <typename T>
hipError_t pooled_rows(const void* qkv, const int* rows, float* out, int B, int S, int H, int causal, const int64_t* key_mask,
                       hipStream_t s) {
  const size_t lds = (size_t)(kDh + S) * sizeof(float);
  hipLaunchKernelGGL(attention_pooled_rows_kernel<T>, dim3(H, B), dim3(kThreads), lds, s, (const T*)qkv, rows, out, S, H, causal, key_mask);
  return hipGetLastError();
}

template <typename T, int RPL>
hipError_t rollout_step_rpl(const void* qkv, const float* R_in, float* R_out, int B, int S, int H, int causal, const int64_t* key_mask,
                            const int* rows, float* pooled_out, hipStream_t s) {
  const size_t lds = attention_rollout_lds_bytes(S);
  const hipError_t e = allow_lds(&attention_rollout_step_kernel<T, RPL>, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((attention_rollout_step_kernel<T, RPL>), dim3((S + kRows - 1) / kRows, B), dim3(kThreads), lds, s, (const T*)qkv,
                     R_in, R_out, S, H, causal, key_mask, rows, pooled_out);
  return hipGetLastError();
}

template <typename T>
hipError_t rollout_step(const void* qkv, const float* R_in, float* R_out, int B, int S, int H, int causal, const int64_t* key_mask,
                        const int* rows, float* pooled_out, hipStream_t s) {
  if (S <= 64) return rollout_step_rpl<T, 4>(qkv, R_in, R_out, B, S, H, causal, key_mask, rows, pooled_out, s);
  if (S <= 128) return rollout_step_rpl<T, 8>(qkv, R_in, R_out, B, S, H, causal, key_mask, rows, pooled_out, s);
  return rollout_step_rpl<T, 16>(qkv, R_in, R_out, B, S, H, causal, key_mask, rows, pooled_out, s);
}

}  // namespace

size_t attention_rollout_lds_bytes(int S) { return (size_t)kRows * (kDh + S + ((S + 3) & ~3)) * sizeof(float); }

hipError_t launch_attention_pooled_rows(const void* qkv, const int* rows, float* out, int dtype, int B, int S, int H, int causal,
                                        const int64_t* key_mask, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  if (S <= 0 || S > 1024 || H <= 0 || B > 65535 || !qkv || !rows || !out) return hipErrorInvalidValue;
  if (dtype != 0 && dtype != 1 && dtype != 2) return hipErrorInvalidValue;
  return with_dtype(dtype, [&](auto tag) { return pooled_rows<decltype(tag)>(qkv, rows, out, B, S, H, causal, key_mask, s); });
}

hipError_t launch_attention_rollout_step(const void* qkv, const float* R_in, float* R_out, int dtype, int B, int S, int H, int causal,
                                         const int64_t* key_mask, hipStream_t s, const int* rows, float* pooled_out) {
  if (B <= 0) return hipSuccess;
  if (S <= 0 || S > 1024 || H <= 0 || B > 65535 || !qkv || !R_out || R_in == R_out || (pooled_out && !rows)) return hipErrorInvalidValue;
  if (dtype != 0 && dtype != 1 && dtype != 2) return hipErrorInvalidValue;
  return with_dtype(dtype, [&](auto tag) {
    return rollout_step<decltype(tag)>(qkv, R_in, R_out, B, S, H, causal, key_mask, rows, pooled_out, s);
  });
}

hipError_t launch_attention_rollout_row(const float* R, const int* rows, float* out, int B, int S, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  if (S <= 0 || !R || !rows || !out) return hipErrorInvalidValue;
  hipLaunchKernelGGL(attention_rollout_row_kernel, dim3(B), dim3(256), 0, s, R, rows, out, S);
  return hipGetLastError();
}

}  // namespace plipmi
