// probe_tile.h -- the embedding tile and everything the three heads on cached embeddings X [N, D] fp32 do with it (probe.hip: the
// one-vs-rest pass and the predict kernel; probe_softmax.hip: the multinomial pass; kmeans.hip: the assignment pass):
//   * ProbeTile<CT>: the 32-row tile of X in LDS, its XOR swizzle, a wave's slice of the second operand in its two forms (load_w / scores:
//     scalar reads of rows of stride D + 1; load_centres / tile_scores: 16-byte reads of rows of stride D) and the phase-1 product of each;
//   * the pieces around it: join_scores, block_sum_to, finish_grad_column, the LDS byte count and attribute (probe_lds_bytes, allow_lds),
//     the streaming passes' workgroup count, the choice of the instantiated tile.
// The walk of the two FIT kernels (fetch, scores, residuals, G += R^T X_tile, the slot store) is text: probe_fit_setup.inc,
// probe_fit_walk.inc and probe_fit_rest.inc.  The kernels that only score (predict, softmax statistics, k-means assignment) each write
// their loop over the groups of 16 columns themselves: a shared form of it, function template or text, changed the instructions of every
// kernel of its unit (profiles/embedding_tile_isa_diff.txt).
// Everything here has internal linkage: each unit compiles its own copy.
#pragma once
#include <algorithm>
#include <climits>
#include <type_traits>

#include "kernels.h"

namespace plipmi {

// 64-column blocks of the LDS row, rounded up to an instantiated tile (probe_dispatch); workgroups along x for N rows at width D
// (both defined in probe.hip)
int probe_col_tiles(int D);
int probe_workgroups(int N, int D);

namespace {

constexpr int kRows = 32;        // rows of X per tile
constexpr int kThreads = 256;    // four waves
constexpr int kGroup = 16;       // problems per MFMA tile

__device__ __forceinline__ int probe_swz(int row) { return ((row & 3) << 4) | (((row >> 2) & 3) << 2); }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the four waves' partial scores of (row r, column rc), o = r * kGroup + rc, in wave order, plus the column's bias
__device__ __forceinline__ float join_scores(const float* zp, int o, float bias) {
  return bias + (((zp[o] + zp[kRows * kGroup + o]) + zp[2 * kRows * kGroup + o]) + zp[3 * kRows * kGroup + o]);
}

// the workgroup's 256 per-thread doubles summed by thread 0 in thread order -> *out (global memory or LDS).  `red` is LDS of 256 doubles
// that no thread still reads.
__device__ __forceinline__ void block_sum_to(double* red, double v, int tid, double* out) {
  red[tid] = v;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int i = 0; i < kThreads; ++i) s += red[i];
    *out = s;
  }
}

template <int CT> struct ProbeTile {
  static constexpr int Dp = 64 * CT;          // LDS row length (floats)
  static constexpr int NV = 2 * CT;           // 16-byte loads per thread and tile
  static constexpr int KS = 4 * CT;           // phase-1 k steps (of 4 columns) per wave
  float4 pre[NV];

  // rows [row0, row0 + 32) of X -> registers (zeros past N and past D)
  __device__ __forceinline__ void fetch(const float* __restrict__ X, int N, int D, long row0, int tid) {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int i = tid + kThreads * j, r = i / (Dp / 4), d = (i - r * (Dp / 4)) * 4;
      const long gr = row0 + r;
      pre[j] = (gr < N && d < D) ? *reinterpret_cast<const float4*>(X + gr * D + d) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  __device__ __forceinline__ void stage(float* xs, int tid) const {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int i = tid + kThreads * j, r = i / (Dp / 4), d = (i - r * (Dp / 4)) * 4;
      *reinterpret_cast<float4*>(&xs[r * Dp + (d ^ probe_swz(r))]) = pre[j];
    }
  }
  // the same without the stop in registers (wide rows, where the registers go to the accumulators; the kernels that only score)
  __device__ __forceinline__ static void direct(const float* __restrict__ X, int N, int D, long row0, int tid, float* xs) {
#pragma unroll 4
    for (int j = 0; j < NV; ++j) {
      const int i = tid + kThreads * j, r = i / (Dp / 4), d = (i - r * (Dp / 4)) * 4;
      const long gr = row0 + r;
      *reinterpret_cast<float4*>(&xs[r * Dp + (d ^ probe_swz(r))]) =
          (gr < N && d < D) ? *reinterpret_cast<const float4*>(X + gr * D + d) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }

  // ---- the scalar operand form: rows of stride D + 1 (WB) ----
  // this wave's slice of W for problems kbase .. kbase + 15: wf[s] = W[kbase + (lane & 15)][4 (wave KS + s) + (lane >> 4)]
  __device__ __forceinline__ static void load_w(float (&wf)[KS], const float* __restrict__ WB, int K, int D, int kbase, int wave, int lane) {
    const int cls = kbase + (lane & 15);
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int d = (wave * KS + s) * 4 + (lane >> 4);
      wf[s] = (cls < K && d < D) ? WB[(size_t)cls * (D + 1) + d] : 0.f;
    }
  }
  // phase 1: this wave's partial Z for the tile's two 16-row blocks -> zp[wave][32][16]
  __device__ __forceinline__ static void scores(const float* xs, const float (&wf)[KS], float* zp, int wave, int lane) {
    f32x4 z0 = {0.f, 0.f, 0.f, 0.f}, z1 = {0.f, 0.f, 0.f, 0.f};
    const int m = lane & 15, k = lane >> 4, sw = probe_swz(m);      // probe_swz(m + 16) == probe_swz(m)
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int d = ((wave * KS + s) * 4 + k) ^ sw;
      z0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xs[m * Dp + d], wf[s], z0, 0, 0, 0);
      z1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xs[(m + 16) * Dp + d], wf[s], z1, 0, 0, 0);
    }
    float* o = zp + wave * (kRows * kGroup);
#pragma unroll
    for (int j = 0; j < 4; ++j) {      // C/D layout: column (problem) = lane & 15, row = 4 (lane >> 4) + j
      o[(4 * k + j) * kGroup + m] = z0[j];
      o[(16 + 4 * k + j) * kGroup + m] = z1[j];
    }
  }

  // ---- the 16-byte operand form: rows of stride D (k-means' centres) ----
  // This wave's slice of the rows kbase .. kbase + 15, 16 bytes per lane and load: wave w owns columns [16 CT w, 16 CT (w + 1)), and lane
  // (n = lane & 15, q = lane >> 4) holds wf[j] = C[kbase + n][16 CT w + 16 j + 4 q .. + 3] -- a row's four lanes read 64 contiguous bytes.
  // Zeros past K and D (D % 4 == 0: a group of four is inside or outside as a whole).
  __device__ __forceinline__ static void load_centres(float4 (&wf)[CT], const float* __restrict__ C, int K, int D, int kbase, int wave, int lane) {
    const int cls = kbase + (lane & 15);
#pragma unroll
    for (int j = 0; j < CT; ++j) {
      const int d = wave * 16 * CT + 16 * j + 4 * (lane >> 4);
      wf[j] = (cls < K && d < D) ? *reinterpret_cast<const float4*>(C + (size_t)cls * D + d) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  // This wave's partial scores of the tile's two 16-row blocks against the slice -> zp[wave][32][16].  The MFMA's k index is free as long
  // as both operands agree on it: k-step 4 j + e of lane (m, q) is column 16 CT w + 16 j + 4 q + e, so the X side too is one 16-byte LDS
  // read per four steps (the swizzle moves whole 16-byte groups).  NOT the scalar form's association of the columns: the two forms give
  // different bits and stay apart.
  __device__ __forceinline__ static void tile_scores(const float* xs, const float4 (&wf)[CT], float* zp, int wave, int lane) {
    f32x4 z0 = {0.f, 0.f, 0.f, 0.f}, z1 = {0.f, 0.f, 0.f, 0.f};
    const int m = lane & 15, q = lane >> 4, sw = probe_swz(m);      // probe_swz(m + 16) == probe_swz(m)
#pragma unroll
    for (int j = 0; j < CT; ++j) {
      const int d = (wave * 16 * CT + 16 * j + 4 * q) ^ sw;
      const float4 a0 = *reinterpret_cast<const float4*>(&xs[m * Dp + d]), a1 = *reinterpret_cast<const float4*>(&xs[(m + 16) * Dp + d]);
      z0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, wf[j].x, z0, 0, 0, 0);
      z1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.x, wf[j].x, z1, 0, 0, 0);
      z0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, wf[j].y, z0, 0, 0, 0);
      z1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.y, wf[j].y, z1, 0, 0, 0);
      z0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.z, wf[j].z, z0, 0, 0, 0);
      z1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.z, wf[j].z, z1, 0, 0, 0);
      z0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.w, wf[j].w, z0, 0, 0, 0);
      z1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.w, wf[j].w, z1, 0, 0, 0);
    }
    float* o = zp + wave * (kRows * kGroup);
#pragma unroll
    for (int i = 0; i < 4; ++i) {        // C/D layout: column (centre) = lane & 15, row = 4 (lane >> 4) + i
      o[(4 * q + i) * kGroup + m] = z0[i];
      o[(16 + 4 * q + i) * kGroup + m] = z1[i];
    }
  }
};

// grad[k][d] = (the workgroups' partial sums: four slices of the nwg slots, each in slot order, then the slices in order, in double) / N
// + alpha W[k][d]; the intercept's (d == D) has no penalty.  The gradient column of both finish kernels: grid (K, ceil((D + 1) / 64)),
// 256 threads = column c = tid & 63 of the block's 64 x slice q = tid >> 6; part_g [nwg][KP][D + 1]; sh is LDS.
__device__ __forceinline__ void finish_grad_column(const float* __restrict__ part_g, int nwg, int KP, const float* __restrict__ WB, int N, int D,
                                                   float alpha, float* __restrict__ grad, double (&sh)[4][64], int c, int q) {
  const int k = blockIdx.x;
  const int d = blockIdx.y * 64 + c;
  double acc = 0.0;
  if (d <= D) {
    const int w0 = (int)((long)nwg * q / 4), w1 = (int)((long)nwg * (q + 1) / 4);
    for (int w = w0; w < w1; ++w) acc += (double)part_g[((size_t)w * KP + k) * (D + 1) + d];
  }
  sh[q][c] = acc;
  __syncthreads();
  if (q == 0 && d <= D) {
    const double s = ((sh[0][c] + sh[1][c]) + sh[2][c]) + sh[3][c];
    const double pen = d < D ? (double)alpha * (double)WB[(size_t)k * (D + 1) + d] : 0.0;
    grad[(size_t)k * (D + 1) + d] = (float)(s / N + pen);
  }
}

// dynamic LDS of a tile kernel in bytes: the tile, the four waves' partial scores, and the kernel's own floats behind them
constexpr size_t probe_lds_bytes(int CT, int extra_floats) { return ((size_t)kRows * 64 * CT + 4 * kRows * kGroup + extra_floats) * 4; }

// lets Kernel use `lds` bytes of dynamic LDS (above the 64 KiB a kernel gets unasked); once per kernel and process
template <auto Kernel> hipError_t allow_lds(size_t lds) {
  static bool done = false;
  if (done) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e == hipSuccess) done = true;
  return e;
}

// workgroups of a streaming pass (softmax statistics, k-means assignment): it keeps no accumulators, two per compute unit hide its loads
inline int probe_stream_workgroups(int N, int D) {
  const long ntiles = ((long)N + kRows - 1) / kRows;
  return (int)std::max<long>(1, std::min<long>(ntiles, 2L * probe_workgroups(INT_MAX, D)));
}

}  // namespace

// run f(std::integral_constant<int, CT>) for the instantiated tile that probe_col_tiles chose
template <typename F> hipError_t probe_dispatch(int ct, F&& f) {
  switch (ct) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 4: return f(std::integral_constant<int, 4>());
    case 6: return f(std::integral_constant<int, 6>());
    case 8: return f(std::integral_constant<int, 8>());
    case 12: return f(std::integral_constant<int, 12>());
    default: return f(std::integral_constant<int, 16>());
  }
}

}  // namespace plipmi
