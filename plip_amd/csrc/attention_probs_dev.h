// attention_probs_dev.h -- the device code attention_probs.hip and attention_summary.hip share: the score tile of one (sample, head,
// block of query rows) into LDS and the row softmax over it, HF eager attention's arithmetic (attention_probs.hip's header comment).
// Every score is one chain of fmaf over the head dim in ascending order and every row's statistics are one wave's reductions,
// whatever the tile shape and however its (row, key) pairs are dealt to the lanes: kernels built from these functions produce the
// same bits for the same (row, key).
#pragma once
#include "kernels.h"

namespace plipmi {
namespace probs_dev {

constexpr int kDh = 64;        // head dim (every CLIP / PLIP variant)
constexpr int kRows = 16;      // query rows per tile
constexpr int kThreads = 256;  // four waves

// q rows i0 .. i0 + rows - 1 of one head (base = the sample's qkv rows at the head's q columns, ld = 3 D) -> qs [R][kDh] fp32;
// tile rows past `rows`: zeros.  The caller synchronises.
template <typename T, int R>
__device__ __forceinline__ void stage_q(float* qs, const T* base, int ld, int i0, int rows, int tid) {
  for (int e = tid; e < R * (kDh / 4); e += kThreads) {
    const int r = e / (kDh / 4), d = (e - r * (kDh / 4)) * 4;
    const float4 v = r < rows ? load4(base + (size_t)(i0 + r) * ld + d) : make_float4(0.f, 0.f, 0.f, 0.f);
    *reinterpret_cast<float4*>(&qs[r * kDh + d]) = v;
  }
}

// phase 1: sc [R][S] = the scores of tile rows i0 .. against every key (masked entries -inf; under the causal mask the keys past
// the tile's last row are not computed).  The workgroup is R / RPL groups of kThreads * RPL / R lanes: a group owns RPL rows of
// the tile, its lanes take one key each.  RPL = R: one key per lane of the workgroup, every row of the tile in that lane's
// registers (long sequences: each k row is read once); a smaller RPL keeps all four waves busy when S is below kThreads.
template <typename T, int R, int RPL>
__device__ __forceinline__ void score_tile(const float* qs, float* sc, const T* base, int ld, int D, int S, int i0, int rows, int b,
                                           int causal, const int64_t* __restrict__ key_mask, int tid) {
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
      for (int d = 0; d < kDh; d += 4) {
        const float4 kv = load4(kr + d);
#pragma unroll
        for (int r = 0; r < RPL; ++r) {
          const float4 qv = *reinterpret_cast<const float4*>(&qs[(r0 + r) * kDh + d]);
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

}  // namespace probs_dev
}  // namespace plipmi
