// attention_probs_dev.h -- the device code attention_probs.hip and attention_summary.hip share: the score tile of one (sample, head,
// block of query rows) into LDS and the row softmax over it, HF eager attention's arithmetic (attention_probs.hip's header comment).
// Every score is one chain of fmaf over the head dim in ascending order and every row's statistics are one wave's reductions,
// whatever the tile shape and however its (row, key) pairs are dealt to the lanes: kernels built from these functions produce the
// same bits for the same (row, key).
// Head size: the functions take DP, the columns a staged q row has in LDS, and `head`, the columns that exist.  DP = kDh is the
// head of 64 with every bound a compile-time constant; the padded sizes 96 and 128 carry heads of 72 .. 128 (the _hd kernels of
// attention_probs.hip / attention_summary.hip): the dot product then runs over `head` columns, so no column past the head is read
// from memory, and the q row's padding is written as zeros.
#pragma once
#include "kernels.h"

namespace plipmi {
namespace probs_dev {

constexpr int kDh = 64;        // head dim of the OpenAI CLIP / PLIP variants
constexpr int kRows = 16;      // query rows per tile
constexpr int kThreads = 256;  // four waves

// q rows i0 .. i0 + rows - 1 of one head (base = the sample's qkv rows at the head's q columns, ld = 3 D) -> qs [R][DP] fp32;
// tile rows past `rows` and columns past `head`: zeros.  The caller synchronises.
template <typename T, int R, int DP = kDh>
__device__ __forceinline__ void stage_q(float* qs, const T* base, int ld, int i0, int rows, int tid, int head = kDh) {
  for (int e = tid; e < R * (DP / 4); e += kThreads) {
    const int r = e / (DP / 4), d = (e - r * (DP / 4)) * 4;
    const float4 v = (r < rows && (DP == kDh || d < head)) ? load4(base + (size_t)(i0 + r) * ld + d) : make_float4(0.f, 0.f, 0.f, 0.f);
    *reinterpret_cast<float4*>(&qs[r * DP + d]) = v;
  }
}

// phase 1: sc [R][S] = the scores of tile rows i0 .. against every key (masked entries -inf; under the causal mask the keys past
// the tile's last row are not computed).  The workgroup is R / RPL groups of kThreads * RPL / R lanes: a group owns RPL rows of
// the tile, its lanes take one key each.  RPL = R: one key per lane of the workgroup, every row of the tile in that lane's
// registers (long sequences: each k row is read once); a smaller RPL keeps all four waves busy when S is below kThreads.
template <typename T, int R, int RPL, int DP = kDh>
__device__ __forceinline__ void score_tile(const float* qs, float* sc, const T* base, int ld, int D, int S, int i0, int rows, int b,
                                           int causal, const int64_t* __restrict__ key_mask, int tid, int head = kDh) {
  static_assert(R % RPL == 0 && kThreads % (R / RPL) == 0, "row groups must divide the tile and the workgroup");
  constexpr int kLanes = kThreads / (R / RPL);           // lanes per row group
  const int r0 = (tid / kLanes) * RPL;                   // the group's first tile row
  const int last_row = i0 + rows - 1;
  const int nkeys = causal ? min(S, last_row + 1) : S;   // keys any row of the tile may attend to
  for (int j = tid % kLanes; j < S; j += kLanes) {
    float acc[RPL];
#pragma unroll
    for (int r = 0; r < RPL; ++r) acc[r] = 0.f;
    const bool live = j < nkeys && (key_mask == nullptr || key_mask[(size_t)b * S + j] != 0);
    if (live) {
      const T* kr = base + (size_t)j * ld + D;
#pragma unroll 4
      for (int d = 0; d < (DP == kDh ? kDh : head); d += 4) {
        const float4 kv = load4(kr + d);
#pragma unroll
        for (int r = 0; r < RPL; ++r) {
          const float4 qv = *reinterpret_cast<const float4*>(&qs[(r0 + r) * DP + d]);
          acc[r] = fmaf(qv.x, kv.x, acc[r]);
          acc[r] = fmaf(qv.y, kv.y, acc[r]);
          acc[r] = fmaf(qv.z, kv.z, acc[r]);
          acc[r] = fmaf(qv.w, kv.w, acc[r]);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < RPL; ++r) sc[(r0 + r) * S + j] = (live && (!causal || j <= i0 + r0 + r)) ? acc[r] : -INFINITY;
  }
}

// phase 2, one wave on one row of the score tile: max and sum by wave reductions, then emit(j, p) for every key j (lane-contiguous),
// p = exp(s - max) / sum; a row with no live key: emit(j, 0) for every j.
template <typename Emit>
__device__ __forceinline__ void softmax_row(const float* sr, int S, int lane, Emit&& emit) {
  float m = -INFINITY;
  for (int j = lane; j < S; j += 64) m = fmaxf(m, sr[j]);
  m = wave_max(m);
  if (m == -INFINITY) {                 // no live key in this row
    for (int j = lane; j < S; j += 64) emit(j, 0.f);
    return;
  }
  float l = 0.f;
  for (int j = lane; j < S; j += 64) l += expf(sr[j] - m);
  const float inv = 1.0f / wave_sum(l);
  for (int j = lane; j < S; j += 64) emit(j, expf(sr[j] - m) * inv);
}

// softmax_row for a caller that may overwrite the score row: exp(s - max) is computed once, kept in the row and scaled afterwards --
// the same p, bit for bit (one expf of the same argument, the same product), for one exponential less per entry.
template <typename Emit>
__device__ __forceinline__ void softmax_row_in_place(float* sr, int S, int lane, Emit&& emit) {
  float m = -INFINITY;
  for (int j = lane; j < S; j += 64) m = fmaxf(m, sr[j]);
  m = wave_max(m);
  if (m == -INFINITY) {                 // no live key in this row
    for (int j = lane; j < S; j += 64) emit(j, 0.f);
    return;
  }
  float l = 0.f;
  for (int j = lane; j < S; j += 64) {
    const float e = expf(sr[j] - m);
    sr[j] = e;
    l += e;
  }
  const float inv = 1.0f / wave_sum(l);
  for (int j = lane; j < S; j += 64) emit(j, sr[j] * inv);
}

// ---- the kernels' bodies, written once for every head size: attention_probs.hip / attention_summary.hip wrap them at DP = kDh
// (their kernels are the instructions they were before the head became a parameter: profiles/head_dim_isa_diff.txt) and, in the
// _hd kernels beside those, at the padded sizes.  Dynamic LDS as each states; what they compute: the kernels' own comments.
// (The rollout step's body is attention_rollout_body.inc, included as text: as a function it came out as other instructions.)

// grid (row blocks, H, B); LDS: qs [kRows][DP], sc [kRows][S]
template <typename T, int DP>
__device__ __forceinline__ void probs_block(const T* qkv, float* probs, int S, int H, int head, int causal,
                                            const int64_t* key_mask) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* qs = lds;                   // [kRows][DP]
  float* sc = lds + kRows * DP;      // [kRows][S]

  const int i0 = blockIdx.x * kRows, h = blockIdx.y, b = blockIdx.z;
  const int D = H * head, ld = 3 * D;
  const int tid = threadIdx.x;
  const int rows = min(kRows, S - i0);
  const T* base = qkv + (size_t)b * S * ld + h * head;

  // q rows of the block -> LDS (rows past S: zeros, never stored)
  stage_q<T, kRows, DP>(qs, base, ld, i0, rows, tid, head);
  __syncthreads();

  // phase 1: scores of every (row, key) of the block, one key per lane
  score_tile<T, kRows, kRows, DP>(qs, sc, base, ld, D, S, i0, rows, b, causal, key_mask, tid, head);
  __syncthreads();

  // phase 2: one wave per row -- softmax statistics, then the normalised row
  const int lane = tid & 63, wave = tid >> 6;
  for (int r = wave; r < rows; r += kThreads / 64) {
    float* pr = probs + (((size_t)b * H + h) * S + (i0 + r)) * S;
    softmax_row(sc + r * S, S, lane, [pr](int j, float p) { pr[j] = p; });
  }
}

// grid (H, B); LDS: qs [1][DP], sc [1][S]
template <typename T, int DP>
__device__ __forceinline__ void pooled_rows_block(const T* qkv, const int* row_idx, float* out,
                                                  int S, int H, int head, int causal, const int64_t* key_mask) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* qs = lds;            // [1][DP]
  float* sc = lds + DP;       // [1][S]
  const int h = blockIdx.x, b = blockIdx.y;
  const int D = H * head, ld = 3 * D;
  const int tid = threadIdx.x;
  const int i0 = min(max(row_idx[b], 0), S - 1);    // (the pooling rule only yields rows of the sequence; a caller's array is clamped)
  const T* base = qkv + (size_t)b * S * ld + h * head;
  stage_q<T, 1, DP>(qs, base, ld, i0, 1, tid, head);
  __syncthreads();
  score_tile<T, 1, 1, DP>(qs, sc, base, ld, D, S, i0, 1, b, causal, key_mask, tid, head);
  __syncthreads();
  if (tid < 64) {
    float* pr = out + ((size_t)b * H + h) * S;
    softmax_row(sc, S, tid, [pr](int j, float p) { pr[j] = p; });
  }
}

// host side: the dynamic LDS of the three bodies at DP staged columns, and the launch of one of their kernels (kThreads lanes per
// workgroup) with the attribute that dynamic LDS past 64 KB needs
inline size_t probs_lds_bytes(int S, int DP) { return (size_t)kRows * (DP + S) * sizeof(float); }
inline size_t pooled_rows_lds_bytes(int S, int DP) { return (size_t)(DP + S) * sizeof(float); }
inline size_t rollout_lds_bytes(int S, int DP) { return (size_t)kRows * (DP + S + ((S + 3) & ~3)) * sizeof(float); }
template <typename... P, typename... A>
inline hipError_t launch_with_lds(void (*kernel)(P...), dim3 grid, size_t lds, hipStream_t s, A... args) {
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kernel, grid, dim3(kThreads), lds, s, static_cast<P>(args)...);
  return hipGetLastError();
}

}  // namespace probs_dev
}  // namespace plipmi
