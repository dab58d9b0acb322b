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
#include "kernels.h"

namespace plipmi {

namespace {

constexpr int kDh = 64;        // head dim (every CLIP / PLIP variant)
constexpr int kRows = 16;      // query rows per workgroup
constexpr int kThreads = 256;  // four waves

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
  for (int e = tid; e < kRows * (kDh / 4); e += kThreads) {
    const int r = e / (kDh / 4), d = (e - r * (kDh / 4)) * 4;
    const float4 v = r < rows ? load4(base + (size_t)(i0 + r) * ld + d) : make_float4(0.f, 0.f, 0.f, 0.f);
    *reinterpret_cast<float4*>(&qs[r * kDh + d]) = v;
  }
  __syncthreads();

  // phase 1: scores of every (row, key) of the block
  const int last_row = i0 + rows - 1;
  const int nkeys = causal ? min(S, last_row + 1) : S;   // keys any row of the block may attend to
  for (int j = tid; j < S; j += kThreads) {
    float acc[kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) acc[r] = 0.f;
    const bool live = j < nkeys && (key_mask == nullptr || key_mask[(size_t)b * S + j] != 0);
    if (live) {
      const T* kr = base + (size_t)j * ld + D;
#pragma unroll 4
      for (int d = 0; d < kDh; d += 4) {
        const float4 kv = load4(kr + d);
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
          const float4 qv = *reinterpret_cast<const float4*>(&qs[r * kDh + d]);
          acc[r] = fmaf(qv.x, kv.x, acc[r]);
          acc[r] = fmaf(qv.y, kv.y, acc[r]);
          acc[r] = fmaf(qv.z, kv.z, acc[r]);
          acc[r] = fmaf(qv.w, kv.w, acc[r]);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < kRows; ++r) sc[r * S + j] = (live && (!causal || j <= i0 + r)) ? acc[r] : -INFINITY;
  }
  __syncthreads();

  // phase 2: one wave per row -- softmax statistics, then the normalised row
  const int lane = tid & 63, wave = tid >> 6;
  for (int r = wave; r < rows; r += kThreads / 64) {
    const float* sr = sc + r * S;
    float m = -INFINITY;
    for (int j = lane; j < S; j += 64) m = fmaxf(m, sr[j]);
    m = wave_max(m);
    float* pr = probs + (((size_t)b * H + h) * S + (i0 + r)) * S;
    if (m == -INFINITY) {                 // no live key in this row
      for (int j = lane; j < S; j += 64) pr[j] = 0.f;
      continue;
    }
    float l = 0.f;
    for (int j = lane; j < S; j += 64) l += expf(sr[j] - m);
    const float inv = 1.0f / wave_sum(l);
    for (int j = lane; j < S; j += 64) pr[j] = expf(sr[j] - m) * inv;
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
#define PLIPMI_PROBS(T)                                                                                                   \
  do {                                                                                                                    \
    if (lds > 64 * 1024) {                                                                                                \
      const hipError_t e_ = hipFuncSetAttribute(reinterpret_cast<const void*>(&attention_probs_kernel<T>),                \
                                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                    \
      if (e_ != hipSuccess) return e_;                                                                                    \
    }                                                                                                                     \
    hipLaunchKernelGGL(attention_probs_kernel<T>, grid, block, lds, s, (const T*)qkv, probs, S, H, causal, key_mask);     \
  } while (0)
  if (dtype == 1) PLIPMI_PROBS(bf16_t);
  else if (dtype == 2) PLIPMI_PROBS(f16_t);
  else if (dtype == 0) PLIPMI_PROBS(float);
  else return hipErrorInvalidValue;
#undef PLIPMI_PROBS
  return hipGetLastError();
}

}  // namespace plipmi
