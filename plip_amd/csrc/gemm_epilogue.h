// gemm_epilogue.h -- the per-element epilogue of the NT GEMM (gemm_nt_kernel's row epilogues and the naive checker).
#pragma once
#include <type_traits>

#include "common.h"
#include "gemm.h"

namespace plipmi {

// Epilogue split in a LOAD half (bias / residual / position rows; issued back to
// back for a whole 32x32 tile so the loads overlap) and a STORE half.
template <typename T, int EPI>
struct EpilogueOp {
  static constexpr bool kAccurate = sizeof(T) == 4;
  using OutT = std::conditional_t<sizeof(T) == 4, float, T>;
  __device__ __forceinline__ static float4 load(const GemmParams& p, int m, int n0) {
    if constexpr (epi_is_colwise(EPI)) {
      return *reinterpret_cast<const float4*>(p.bias + n0);
    } else if constexpr (EPI == EPI_RESID_SPLIT) {
      return make_float4(0.f, 0.f, 0.f, 0.f);   // the split-plane epilogue loads its planes itself (16-byte pieces)
    } else if constexpr (epi_is_resid(EPI)) {
      const float4 b = *reinterpret_cast<const float4*>(p.bias + n0);
      const float4 r = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(p.C) + (size_t)m * p.ldc + n0);
      return make_float4(r.x + b.x, r.y + b.y, r.z + b.z, r.w + b.w);
    } else if constexpr (EPI == EPI_PATCH) {
      const int img = m / p.np, pp = m - img * p.np;
      return *reinterpret_cast<const float4*>(p.bias + (size_t)(1 + pp) * p.N + n0);
    } else {
      return make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  // 4 consecutive columns n0..n0+3 of output row m
  __device__ __forceinline__ static void store(const GemmParams& p, int m, int n0, float v0, float v1, float v2,
                                               float v3, const float4 add) {
    if constexpr (epi_is_colwise(EPI)) {
      v0 += add.x; v1 += add.y; v2 += add.z; v3 += add.w;
      if constexpr (EPI == EPI_BIAS_QGELU) {
        v0 = quick_gelu<kAccurate>(v0); v1 = quick_gelu<kAccurate>(v1);
        v2 = quick_gelu<kAccurate>(v2); v3 = quick_gelu<kAccurate>(v3);
      } else if constexpr (EPI == EPI_BIAS_GELU) {
        v0 = erf_gelu<kAccurate>(v0); v1 = erf_gelu<kAccurate>(v1);
        v2 = erf_gelu<kAccurate>(v2); v3 = erf_gelu<kAccurate>(v3);
      }
      store4(reinterpret_cast<OutT*>(p.C) + (size_t)m * p.ldc + n0, v0, v1, v2, v3);
    } else if constexpr (epi_is_resid(EPI)) {
      store4(reinterpret_cast<float*>(p.C) + (size_t)m * p.ldc + n0, add.x + v0, add.y + v1, add.z + v2, add.w + v3);
    } else if constexpr (EPI == EPI_SCALE) {
      store4(reinterpret_cast<float*>(p.C) + (size_t)m * p.ldc + n0, p.alpha * v0, p.alpha * v1, p.alpha * v2,
             p.alpha * v3);
    } else {  // EPI_PATCH: patch row m = img*np + pp goes to token row img*(np+1) + 1 + pp
      const int img = m / p.np, pp = m - img * p.np;
      float* c = reinterpret_cast<float*>(p.C) + ((size_t)img * (p.np + 1) + 1 + pp) * p.ldc + n0;
      store4(c, v0 + add.x, v1 + add.y, v2 + add.z, v3 + add.w);
    }
  }
};

// The column-wise 16-bit epilogue's arithmetic on four accumulator values of one row, the same for both MFMA layouts:
// y = [rstd *] c + bias, [QuickGELU / GELU], rounded to the output type.
template <typename OutT, int EPI>
__device__ __forceinline__ typename half_traits<OutT>::x4 finish_colwise(float c0, float c1, float c2, float c3, float rs, const float4 bias) {
  float v0, v1, v2, v3;
  if constexpr (epi_is_ln(EPI)) {
    v0 = fmaf(rs, c0, bias.x); v1 = fmaf(rs, c1, bias.y);
    v2 = fmaf(rs, c2, bias.z); v3 = fmaf(rs, c3, bias.w);
  } else {
    v0 = c0 + bias.x; v1 = c1 + bias.y; v2 = c2 + bias.z; v3 = c3 + bias.w;
  }
  if constexpr (EPI == EPI_BIAS_QGELU || EPI == EPI_QGELU_LN) {
    v0 = quick_gelu<false>(v0); v1 = quick_gelu<false>(v1);
    v2 = quick_gelu<false>(v2); v3 = quick_gelu<false>(v3);
  } else if constexpr (EPI == EPI_BIAS_GELU || EPI == EPI_GELU_LN) {
    v0 = erf_gelu<false>(v0); v1 = erf_gelu<false>(v1);
    v2 = erf_gelu<false>(v2); v3 = erf_gelu<false>(v3);
  }
  return {from_f32<OutT>(v0), from_f32<OutT>(v1), from_f32<OutT>(v2), from_f32<OutT>(v3)};
}

}  // namespace plipmi
