// probe_tile.h -- what the linear-probe kernels share (probe.hip: the one-vs-rest pass and the predict kernel; probe_softmax.hip:
// the multinomial pass): the 32-row tile of X in LDS, its XOR swizzle, a wave's slice of W and the phase-1 product, and the choice of
// the instantiated tile.  Everything here has internal linkage: each unit compiles its own copy.
#pragma once
#include <type_traits>

#include "kernels.h"

namespace plipmi {

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
  // the same without the stop in registers (wide rows, where the registers go to the accumulators; the predict kernel)
  __device__ __forceinline__ static void direct(const float* __restrict__ X, int N, int D, long row0, int tid, float* xs) {
#pragma unroll 4
    for (int j = 0; j < NV; ++j) {
      const int i = tid + kThreads * j, r = i / (Dp / 4), d = (i - r * (Dp / 4)) * 4;
      const long gr = row0 + r;
      *reinterpret_cast<float4*>(&xs[r * Dp + (d ^ probe_swz(r))]) =
          (gr < N && d < D) ? *reinterpret_cast<const float4*>(X + gr * D + d) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
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
};

}  // namespace

// 64-column blocks of the LDS row, rounded up to an instantiated tile (probe_dispatch); workgroups along x for N rows at width D
// (both defined in probe.hip)
int probe_col_tiles(int D);
int probe_workgroups(int N, int D);

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
