// kernels.hip -- the HBM-bound kernels around the GEMMs: LayerNorm, patch unfold,
// embeddings, pooled projection head, L2 normalise, logits, top-k, weight packing.
// All are wavefront(64)-shaped: one wave per row for row reductions (shuffle/DPP
// reductions, no LDS), 16-byte accesses per lane, fp32 statistics.
#include <limits.h>

#include "kernels.h"

namespace plipmi {

// ---------------------------------------------------------------------------------
// LayerNorm (nn.LayerNorm, biased variance; modeling_clip.py:358,360,559,605,608)
// ---------------------------------------------------------------------------------
constexpr int kLnMaxVec = 8;  // float4 per lane -> D <= 2048

template <typename TOut>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* x, size_t xs,  // x may alias y (in-place pre-LN)
                                                        const float* __restrict__ g, const float* __restrict__ b,
                                                        TOut* y, int rows, int D, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = x + (size_t)row * xs;
  float4 v[kLnMaxVec];
  float s = 0.f;
#pragma unroll
  for (int it = 0; it < kLnMaxVec; ++it) {
    const int idx = it * 256 + lane * 4;
    if (idx < D) {
      v[it] = *reinterpret_cast<const float4*>(xr + idx);
      s += (v[it].x + v[it].y) + (v[it].z + v[it].w);
    }
  }
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int it = 0; it < kLnMaxVec; ++it) {
    const int idx = it * 256 + lane * 4;
    if (idx < D) {
      const float a = v[it].x - mean, c = v[it].y - mean, d = v[it].z - mean, e = v[it].w - mean;
      q += (a * a + c * c) + (d * d + e * e);
    }
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
  TOut* yr = y + (size_t)row * D;
#pragma unroll
  for (int it = 0; it < kLnMaxVec; ++it) {
    const int idx = it * 256 + lane * 4;
    if (idx < D) {
      const float4 gg = *reinterpret_cast<const float4*>(g + idx);
      const float4 bb = *reinterpret_cast<const float4*>(b + idx);
      store4(yr + idx, (v[it].x - mean) * rstd * gg.x + bb.x, (v[it].y - mean) * rstd * gg.y + bb.y,
             (v[it].z - mean) * rstd * gg.z + bb.z, (v[it].w - mean) * rstd * gg.w + bb.w);
    }
  }
}

// D == NV * 256 exactly (CLIP widths 512 / 768 / 1024): no per-chunk predicates, RPW rows per wave so that RPW * NV
// 16-byte loads per lane are in flight before the first reduction starts, gamma / beta fetched once per wave.
template <typename TOut, int NV, int RPW>
__global__ __launch_bounds__(256) void layernorm_fixed_kernel(const float* x, size_t xs, const float* __restrict__ g,
                                                              const float* __restrict__ b, TOut* y, int rows, float eps) {
  constexpr int D = NV * 256;
  const int lane = threadIdx.x & 63;
  const int row0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW;
  if (row0 >= rows) return;
  float4 v[RPW][NV];
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const int row = row0 + r < rows ? row0 + r : rows - 1;
#pragma unroll
    for (int it = 0; it < NV; ++it) v[r][it] = *reinterpret_cast<const float4*>(x + (size_t)row * xs + it * 256 + lane * 4);
  }
  float4 gg[NV], bb[NV];
#pragma unroll
  for (int it = 0; it < NV; ++it) {
    gg[it] = *reinterpret_cast<const float4*>(g + it * 256 + lane * 4);
    bb[it] = *reinterpret_cast<const float4*>(b + it * 256 + lane * 4);
  }
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    float s = 0.f;
#pragma unroll
    for (int it = 0; it < NV; ++it) s += (v[r][it].x + v[r][it].y) + (v[r][it].z + v[r][it].w);
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int it = 0; it < NV; ++it) {
      const float a = v[r][it].x - mean, c = v[r][it].y - mean, d = v[r][it].z - mean, e = v[r][it].w - mean;
      q += (a * a + c * c) + (d * d + e * e);
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
    if (row0 + r < rows) {
      TOut* yr = y + (size_t)(row0 + r) * D;
#pragma unroll
      for (int it = 0; it < NV; ++it)
        store4(yr + it * 256 + lane * 4, (v[r][it].x - mean) * rstd * gg[it].x + bb[it].x,
               (v[r][it].y - mean) * rstd * gg[it].y + bb[it].y, (v[r][it].z - mean) * rstd * gg[it].z + bb[it].z,
               (v[r][it].w - mean) * rstd * gg[it].w + bb[it].w);
    }
  }
}

// ---------------------------------------------------------------------------------
// LayerNorm folded into the neighbouring GEMMs (bf16 engine; gemm.h EPI_*_LN / EPI_RESID_EMIT).
//   * layernorm_emit_kernel: the ONE LayerNorm pass a tower keeps (vision pre_layrnorm, modeling_clip.py:642): reads the
//     fp32 embedding rows, writes the normalised rows as the engine's split residual stream (common.h split_f32: the hi
//     plane is the bf16 A operand of the q/k/v GEMM, hi + the 8-bit lo plane the stream at 16 / 19 significand bits) and the rows' statistics as
//     per-64-column partials {sum, centred M2} for the first block's folded LayerNorm.
//   * fold_ln_kernel (plipmi_create): W'[n,:] = bf16(pre * (W[n,:] * g - mean_k(W[n,:] * g))) -- gain folded in and the
//     row centred, so that x . W'^T == (x - mean(x)) . (W * g)^T and LayerNorm's mean subtraction needs no epilogue term;
//     c2[n] = pre * (sum_k W[n,k] b[k] + bias[n]); sums in fp64.
// ---------------------------------------------------------------------------------
template <typename H>
__global__ __launch_bounds__(256) void layernorm_emit_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                             const float* __restrict__ b, unsigned short* __restrict__ hi,
                                                             unsigned char* __restrict__ lo, float* __restrict__ st, int rows,
                                                             int D, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;                       // wave-uniform
  const float* xr = x + (size_t)row * D;
  float4 v[kLnMaxVec];
  float s = 0.f;
#pragma unroll
  for (int it = 0; it < kLnMaxVec; ++it) {
    const int idx = it * 256 + lane * 4;
    v[it] = idx < D ? *reinterpret_cast<const float4*>(xr + idx) : make_float4(0.f, 0.f, 0.f, 0.f);
    s += (v[it].x + v[it].y) + (v[it].z + v[it].w);
  }
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int it = 0; it < kLnMaxVec; ++it) {
    const int idx = it * 256 + lane * 4;
    if (idx < D) {
      const float a = v[it].x - mean, c = v[it].y - mean, d = v[it].z - mean, e = v[it].w - mean;
      q += (a * a + c * c) + (d * d + e * e);
    }
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
  const int ns = D / kLnSlice;
#pragma unroll
  for (int it = 0; it < kLnMaxVec; ++it) {
    const int idx = it * 256 + lane * 4;       // 16 lanes = one 64-column slice (D % 64 == 0)
    if (it * 256 >= D) break;                    // wave-uniform: every lane runs the DPP reductions of a live chunk
    const bool live = idx < D;
    float4 y = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) {
      const float4 gg = *reinterpret_cast<const float4*>(g + idx);
      const float4 bb = *reinterpret_cast<const float4*>(b + idx);
      y = make_float4((v[it].x - mean) * rstd * gg.x + bb.x, (v[it].y - mean) * rstd * gg.y + bb.y,
                      (v[it].z - mean) * rstd * gg.z + bb.z, (v[it].w - mean) * rstd * gg.w + bb.w);
    }
    const float ssum = row16_sum((y.x + y.y) + (y.z + y.w));
    const float mj = ssum * (1.0f / kLnSlice);
    const float d0 = y.x - mj, d1 = y.y - mj, d2 = y.z - mj, d3 = y.w - mj;
    const float m2 = row16_sum((d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3));
    if (live) {
      store4_split<H>(hi, lo, (size_t)row, (unsigned)idx, (unsigned)D, y.x, y.y, y.z, y.w);
      if ((lane & 15) == 0) *reinterpret_cast<float2*>(st + ((size_t)row * ns + idx / kLnSlice) * 2) = make_float2(ssum, m2);
    }
  }
}
hipError_t launch_layernorm_emit(const float* x, const float* g, const float* b, void* hi, void* lo, float* st, int rows, int D,
                                 float eps, int dtype, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (D % kLnSlice || D > kLnMaxVec * 256 || (dtype != 1 && dtype != 2)) return hipErrorInvalidValue;
  if (dtype == 1)
    hipLaunchKernelGGL(layernorm_emit_kernel<bf16_t>, dim3((rows + 3) / 4), dim3(256), 0, s, x, g, b, (unsigned short*)hi,
                       (unsigned char*)lo, st, rows, D, eps);
  else
    hipLaunchKernelGGL(layernorm_emit_kernel<f16_t>, dim3((rows + 3) / 4), dim3(256), 0, s, x, g, b, (unsigned short*)hi,
                       (unsigned char*)lo, st, rows, D, eps);
  return hipGetLastError();
}

// hi/lo planes -> plain fp32 rows (plipmi_debug_hidden, and the head of an engine that runs its last block on every token)
template <typename H>
__global__ __launch_bounds__(256) void join_planes_kernel(const unsigned short* __restrict__ hi, const unsigned char* __restrict__ lo,
                                                          float* __restrict__ x, size_t n4, unsigned D) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const size_t m = i * 4 / D;
  *reinterpret_cast<float4*>(x + i * 4) = load4_split<H>(hi, lo, m, (unsigned)(i * 4 - m * D), D);
}
hipError_t launch_join_planes(const void* hi, const void* lo, float* x, size_t rows, int D, int dtype, hipStream_t s) {
  const size_t n = rows * (size_t)D;
  if (n == 0) return hipSuccess;
  if (D % 8 || (dtype != 1 && dtype != 2)) return hipErrorInvalidValue;
  if (dtype == 1)
    hipLaunchKernelGGL(join_planes_kernel<bf16_t>, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, s, (const unsigned short*)hi,
                       (const unsigned char*)lo, x, n / 4, (unsigned)D);
  else
    hipLaunchKernelGGL(join_planes_kernel<f16_t>, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, s, (const unsigned short*)hi,
                       (const unsigned char*)lo, x, n / 4, (unsigned)D);
  return hipGetLastError();
}

// the residual planes from one operand type's split format to the other's, in place: the value is joined in the old code and split
// again in the new one (the new hi = the value rounded to the new operand type -- the next block's A operand -- and a new 8-bit
// remainder: one more rounding of the stream at 2^-16 / 2^-19 relative, common.h split_f32)
template <typename HF, typename HT>
__global__ __launch_bounds__(256) void recode_planes_kernel(unsigned short* __restrict__ hi, unsigned char* __restrict__ lo, size_t n4, unsigned D) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const size_t m = i * 4 / D;
  const unsigned n = (unsigned)(i * 4 - m * D);
  const float4 v = load4_split<HF>(hi, lo, m, n, D);
  store4_split<HT>(hi, lo, m, n, D, v.x, v.y, v.z, v.w);
}
hipError_t launch_recode_planes(void* hi, void* lo, size_t rows, int D, int from_dtype, int to_dtype, hipStream_t s) {
  const size_t n = rows * (size_t)D;
  if (n == 0 || from_dtype == to_dtype) return hipSuccess;
  if (D % 8 || (from_dtype != 1 && from_dtype != 2) || (to_dtype != 1 && to_dtype != 2)) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((n / 4 + 255) / 256));
  if (from_dtype == 2)
    hipLaunchKernelGGL((recode_planes_kernel<f16_t, bf16_t>), grid, dim3(256), 0, s, (unsigned short*)hi, (unsigned char*)lo, n / 4, (unsigned)D);
  else
    hipLaunchKernelGGL((recode_planes_kernel<bf16_t, f16_t>), grid, dim3(256), 0, s, (unsigned short*)hi, (unsigned char*)lo, n / 4, (unsigned)D);
  return hipGetLastError();
}

template <typename H>
__global__ __launch_bounds__(256) void fold_ln_kernel(const float* __restrict__ W, const float* __restrict__ bias,
                                                      const float* __restrict__ g, const float* __restrict__ b,
                                                      H* __restrict__ Wf, float* __restrict__ c2, int rows, int K,
                                                      float pre) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* wr = W + (size_t)row * K;
  // pass 1: mean over k of W[n,k] * g[k] (what centring the row removes), and W[n,:] . b
  double s1 = 0.0, s2 = 0.0;
  for (int k = lane * 4; k < K; k += 256) {
    const float4 w = *reinterpret_cast<const float4*>(wr + k);
    const float4 gg = *reinterpret_cast<const float4*>(g + k);
    const float4 bb = *reinterpret_cast<const float4*>(b + k);
    s1 += ((double)w.x * gg.x + (double)w.y * gg.y) + ((double)w.z * gg.z + (double)w.w * gg.w);
    s2 += ((double)w.x * bb.x + (double)w.y * bb.y) + ((double)w.z * bb.z + (double)w.w * bb.w);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64); }
  const float wmean = (float)(s1 / (double)K);
  // pass 2: the folded, centred, scaled row in bf16
  for (int k = lane * 4; k < K; k += 256) {
    const float4 w = *reinterpret_cast<const float4*>(wr + k);
    const float4 gg = *reinterpret_cast<const float4*>(g + k);
    store4(Wf + (size_t)row * K + k, pre * (w.x * gg.x - wmean), pre * (w.y * gg.y - wmean), pre * (w.z * gg.z - wmean),
           pre * (w.w * gg.w - wmean));
  }
  if (lane == 0) c2[row] = (float)((double)pre * (s2 + (double)bias[row]));
}
hipError_t launch_fold_ln(const float* W, const float* bias, const float* g, const float* b, void* Wf, float* c2, int rows,
                          int K, float pre, int dtype, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (K % 4 || (dtype != 1 && dtype != 2)) return hipErrorInvalidValue;
  if (dtype == 1) hipLaunchKernelGGL(fold_ln_kernel<bf16_t>, dim3((rows + 3) / 4), dim3(256), 0, s, W, bias, g, b, (bf16_t*)Wf, c2, rows, K, pre);
  else hipLaunchKernelGGL(fold_ln_kernel<f16_t>, dim3((rows + 3) / 4), dim3(256), 0, s, W, bias, g, b, (f16_t*)Wf, c2, rows, K, pre);
  return hipGetLastError();
}

hipError_t launch_layernorm(const float* x, size_t xs, const float* g, const float* b, void* y, int y_dtype, int rows,
                            int D, float eps, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (D % 4 || D > kLnMaxVec * 256) return hipErrorInvalidValue;
  if (y_dtype != 0 && (D == 512 || D == 768 || D == 1024)) {  // one kernel for every batch size: batch invariance is bitwise
    constexpr int RPW = 2;
    const dim3 grid((rows + 4 * RPW - 1) / (4 * RPW)), block(256);
#define PLIPMI_LNF(H) \
    if (D == 512) hipLaunchKernelGGL((layernorm_fixed_kernel<H, 2, RPW>), grid, block, 0, s, x, xs, g, b, (H*)y, rows, eps); \
    else if (D == 768) hipLaunchKernelGGL((layernorm_fixed_kernel<H, 3, RPW>), grid, block, 0, s, x, xs, g, b, (H*)y, rows, eps); \
    else hipLaunchKernelGGL((layernorm_fixed_kernel<H, 4, RPW>), grid, block, 0, s, x, xs, g, b, (H*)y, rows, eps)
    if (y_dtype == 1) { PLIPMI_LNF(bf16_t); } else { PLIPMI_LNF(f16_t); }
#undef PLIPMI_LNF
    return hipGetLastError();
  }
  const dim3 grid((rows + 3) / 4), block(256);
  if (y_dtype == 1)
    hipLaunchKernelGGL(layernorm_kernel<bf16_t>, grid, block, 0, s, x, xs, g, b, (bf16_t*)y, rows, D, eps);
  else if (y_dtype == 2)
    hipLaunchKernelGGL(layernorm_kernel<f16_t>, grid, block, 0, s, x, xs, g, b, (f16_t*)y, rows, D, eps);
  else
    hipLaunchKernelGGL(layernorm_kernel<float>, grid, block, 0, s, x, xs, g, b, (float*)y, rows, D, eps);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------
// Patch unfold: Conv2d(kernel = stride = P) is a pure re-index (modeling_clip.py:148-154,
// 209-210): row (img, gi, gj), column (c, u, v) -- the order of conv.weight.reshape(out,-1).
// ---------------------------------------------------------------------------------
template <typename TOut, bool kVec>
__global__ __launch_bounds__(256) void unfold_kernel(const float* __restrict__ px, TOut* __restrict__ out, int H, int W,
                                                     int P, int K, int Kpad) {
  const int gh = H / P, gw = W / P;
  const int row = blockIdx.x;  // img*gh*gw + gi*gw + gj
  const int img = row / (gh * gw), cell = row - img * gh * gw, gi = cell / gw, gj = cell - gi * gw;
  const float* base = px + (size_t)img * 3 * H * W + (size_t)(gi * P) * W + gj * P;
  TOut* orow = out + (size_t)row * Kpad;
  for (int k = threadIdx.x * 4; k < Kpad; k += 256 * 4) {
    float r[4];
    if constexpr (kVec) {  // P % 4 == 0: the 4 columns are 4 consecutive pixels of one image row
      if (k < K) {
        const int c = k / (P * P), rem = k - c * P * P, u = rem / P, v = rem - u * P;
        const float4 t = *reinterpret_cast<const float4*>(base + (size_t)c * H * W + (size_t)u * W + v);
        r[0] = t.x; r[1] = t.y; r[2] = t.z; r[3] = t.w;
      } else {
        r[0] = r[1] = r[2] = r[3] = 0.f;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int kk = k + e;
        if (kk < K) {
          const int c = kk / (P * P), rem = kk - c * P * P, u = rem / P, v = rem - u * P;
          r[e] = base[(size_t)c * H * W + (size_t)u * W + v];
        } else {
          r[e] = 0.f;
        }
      }
    }
    store4(orow + k, r[0], r[1], r[2], r[3]);
  }
}

hipError_t launch_unfold_patches(const float* pixels, void* out, int out_dtype, int B, int H, int W, int patch, int Kpad,
                                 hipStream_t s) {
  if (B <= 0) return hipSuccess;
  const int K = 3 * patch * patch;
  const dim3 grid(B * (H / patch) * (W / patch)), block(256);
  const bool vec = (patch % 4 == 0) && (W % 4 == 0) && (H * W) % 4 == 0;   // every float4 load 16-byte aligned
#define PLIPMI_UNFOLD(T, V) \
  hipLaunchKernelGGL((unfold_kernel<T, V>), grid, block, 0, s, pixels, (T*)out, H, W, patch, K, Kpad)
  if (out_dtype == 1) { if (vec) PLIPMI_UNFOLD(bf16_t, true); else PLIPMI_UNFOLD(bf16_t, false); }
  else if (out_dtype == 2) { if (vec) PLIPMI_UNFOLD(f16_t, true); else PLIPMI_UNFOLD(f16_t, false); }
  else                { if (vec) PLIPMI_UNFOLD(float, true);  else PLIPMI_UNFOLD(float, false); }
#undef PLIPMI_UNFOLD
  return hipGetLastError();
}

// uint8 HWC tiles: one thread produces 4 consecutive v of one (c,u) row = 4 pixels -> reads 4 x 3 bytes (12 contiguous).
// Normalisation constants: CLIP mean/std (transform.py:50; HF CLIPImageProcessor defaults).
template <typename TOut>
__global__ __launch_bounds__(256) void unfold_u8_kernel(const uint8_t* __restrict__ px, TOut* __restrict__ out, int H, int W,
                                                        int P, int K, int Kpad) {
  const float mean[3] = {0.48145466f, 0.4578275f, 0.40821073f};
  const float istd[3] = {1.0f / 0.26862954f, 1.0f / 0.26130258f, 1.0f / 0.27577711f};
  const int gh = H / P, gw = W / P;
  const int row = blockIdx.x;
  const int img = row / (gh * gw), cell = row - img * gh * gw, gi = cell / gw, gj = cell - gi * gw;
  const uint8_t* base = px + ((size_t)img * H * W + (size_t)(gi * P) * W + gj * P) * 3;
  TOut* orow = out + (size_t)row * Kpad;
  for (int k = threadIdx.x * 4; k < Kpad; k += 256 * 4) {
    float r[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int kk = k + e;
      if (kk < K) {
        const int c = kk / (P * P), rem = kk - c * P * P, u = rem / P, v = rem - u * P;
        const float x = (float)base[((size_t)u * W + v) * 3 + c] / 255.0f;   // same op order as the reference
        r[e] = (x - mean[c]) * istd[c];
      } else {
        r[e] = 0.f;
      }
    }
    store4(orow + k, r[0], r[1], r[2], r[3]);
  }
}
hipError_t launch_unfold_patches_u8(const uint8_t* tiles, void* out, int out_dtype, int B, int H, int W, int patch,
                                    int Kpad, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  const int K = 3 * patch * patch;
  const dim3 grid(B * (H / patch) * (W / patch)), block(256);
  if (out_dtype == 1)
    hipLaunchKernelGGL(unfold_u8_kernel<bf16_t>, grid, block, 0, s, tiles, (bf16_t*)out, H, W, patch, K, Kpad);
  else if (out_dtype == 2)
    hipLaunchKernelGGL(unfold_u8_kernel<f16_t>, grid, block, 0, s, tiles, (f16_t*)out, H, W, patch, K, Kpad);
  else
    hipLaunchKernelGGL(unfold_u8_kernel<float>, grid, block, 0, s, tiles, (float*)out, H, W, patch, K, Kpad);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------
// Position table at another grid (modeling_clip.py CLIPVisionEmbeddings.interpolate_pos_encoding): aten's
// upsample_bicubic2d with align_corners = False and an explicit output size -- scale = (float)n0 / g,
// real = scale * (dst + 0.5) - 0.5 (not clamped for cubic), i = floor(real), t = real - i, Keys weights with A = -0.75,
// taps i-1 .. i+2 clamped to [0, n0-1]; the four rows are interpolated along x, then the four results along y.
// One thread per (output row, column d): reads are coalesced over d.  Runs once per derived handle (plipmi_clone_resolution).
// ---------------------------------------------------------------------------------
__device__ __forceinline__ void cubic_weights(float t, float w[4]) {
  const float A = -0.75f;
  auto c1 = [&](float x) { return ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f; };          // |x| <= 1
  auto c2 = [&](float x) { return ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A; };    // 1 < |x| < 2
  w[0] = c2(t + 1.f); w[1] = c1(t); w[2] = c1(1.f - t); w[3] = c2(2.f - t);
}

__global__ __launch_bounds__(256) void resample_pos_kernel(const float* __restrict__ src, float* __restrict__ dst, int n0, int gh,
                                                           int gw, int D) {
  const int row = blockIdx.y;                         // 0 = CLS, 1 + y * gw + x = patch (y, x)
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d >= D) return;
  if (row == 0) { dst[d] = src[d]; return; }
  const int y = (row - 1) / gw, x = (row - 1) - y * gw;
  const float sy = (float)n0 / (float)gh, sx = (float)n0 / (float)gw;
  const float ry = sy * ((float)y + 0.5f) - 0.5f, rx = sx * ((float)x + 0.5f) - 0.5f;
  const int iy = (int)floorf(ry), ix = (int)floorf(rx);
  float wy[4], wx[4];
  cubic_weights(ry - (float)iy, wy);
  cubic_weights(rx - (float)ix, wx);
  const float* tab = src + D;                         // the n0 x n0 patch rows
  float acc = 0.f;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int yy = min(max(iy - 1 + a, 0), n0 - 1);
    float r[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) r[b] = tab[((size_t)yy * n0 + min(max(ix - 1 + b, 0), n0 - 1)) * D + d];
    const float v = r[0] * wx[0] + r[1] * wx[1] + r[2] * wx[2] + r[3] * wx[3];
    acc = a == 0 ? v * wy[0] : acc + v * wy[a];
  }
  dst[(size_t)row * D + d] = acc;
}

hipError_t launch_resample_pos(const float* src, float* dst, int n0, int gh, int gw, int D, hipStream_t s) {
  if (n0 <= 0 || gh <= 0 || gw <= 0 || D <= 0 || src == dst) return hipErrorInvalidValue;
  hipLaunchKernelGGL(resample_pos_kernel, dim3((D + 255) / 256, 1 + gh * gw), dim3(256), 0, s, src, dst, n0, gh, gw, D);
  return hipGetLastError();
}

// x[b,0,:] = class_embedding + position_embedding[0]   (modeling_clip.py:212-217)
__global__ void cls_rows_kernel(const float* __restrict__ cls, const float* __restrict__ pos, float* __restrict__ x,
                                int tokens, int D) {
  float* xr = x + (size_t)blockIdx.x * tokens * D;
  for (int i = threadIdx.x * 4; i < D; i += blockDim.x * 4) {
    const float4 a = *reinterpret_cast<const float4*>(cls + i), p = *reinterpret_cast<const float4*>(pos + i);
    store4(xr + i, a.x + p.x, a.y + p.y, a.z + p.z, a.w + p.w);
  }
}
hipError_t launch_cls_rows(const float* cls, const float* pos, float* x, int B, int tokens, int D, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(cls_rows_kernel, dim3(B), dim3(256), 0, s, cls, pos, x, tokens, D);
  return hipGetLastError();
}

// x[b,s,:] = token_embedding[ids[b,s]] + position_embedding[s]   (modeling_clip.py:251-254)
// A token id outside [0, vocab): the reference's embedding lookup raises (plip.py:68 -> HF nn.Embedding; on a GPU as a
// device-side assert that surfaces at the next synchronisation).  Here the lookup is clamped so that no wild address is
// read, and *bad_id -- a flag in host-visible memory owned by the handle -- is raised; the engine reports it at the
// next call / plipmi_check_async (engine.hip).
__device__ __forceinline__ long long checked_token(long long id, int vocab, int* bad_id, int lane) {
  if (id >= 0 && id < vocab) return id;
  if (bad_id && lane == 0) *bad_id = 1;
  return id < 0 ? 0 : vocab - 1;
}
__global__ void text_embed_kernel(const int64_t* __restrict__ ids, const float* __restrict__ tok,
                                  const float* __restrict__ pos, float* __restrict__ x, int S, int D, int vocab,
                                  int* __restrict__ bad_id) {
  const int row = blockIdx.x;
  long long id = ids[row];
  id = checked_token(id, vocab, bad_id, threadIdx.x);
  const float* t = tok + (size_t)id * D;
  const float* p = pos + (size_t)(row % S) * D;
  float* xr = x + (size_t)row * D;
  for (int i = threadIdx.x * 4; i < D; i += blockDim.x * 4) {
    const float4 a = *reinterpret_cast<const float4*>(t + i), b = *reinterpret_cast<const float4*>(p + i);
    store4(xr + i, a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
  }
}
hipError_t launch_text_embed(const int64_t* ids, const float* tok, const float* pos, float* x, int B, int S, int D,
                             int vocab, int* bad_id, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(text_embed_kernel, dim3(B * S), dim3(128), 0, s, ids, tok, pos, x, S, D, vocab, bad_id);
  return hipGetLastError();
}

// the same lookup for the LayerNorm-folded engine: writes the rows as the split residual stream (hi/lo planes) and emits
// their statistics partials (one wave per row; 16 lanes cover one 64-column slice)
template <typename H>
__global__ __launch_bounds__(256) void text_embed_emit_kernel(const int64_t* __restrict__ ids, const float* __restrict__ tok,
                                                              const float* __restrict__ pos, unsigned short* __restrict__ hi,
                                                              unsigned char* __restrict__ lo, float* __restrict__ st, int rows,
                                                              int S, int D, int vocab, int* __restrict__ bad_id) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  long long id = ids[row];
  id = checked_token(id, vocab, bad_id, lane);
  const float* t = tok + (size_t)id * D;
  const float* p = pos + (size_t)(row % S) * D;
  const int ns = D / kLnSlice;
  for (int c0 = 0; c0 < D; c0 += 256) {          // wave-uniform trip count
    const int idx = c0 + lane * 4;
    const bool live = idx < D;
    float4 y = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) {
      const float4 a = *reinterpret_cast<const float4*>(t + idx), b = *reinterpret_cast<const float4*>(p + idx);
      y = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
    }
    const float ssum = row16_sum((y.x + y.y) + (y.z + y.w));
    const float mj = ssum * (1.0f / kLnSlice);
    const float d0 = y.x - mj, d1 = y.y - mj, d2 = y.z - mj, d3 = y.w - mj;
    const float m2 = row16_sum((d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3));
    if (live) {
      store4_split<H>(hi, lo, (size_t)row, (unsigned)idx, (unsigned)D, y.x, y.y, y.z, y.w);
      if ((lane & 15) == 0) *reinterpret_cast<float2*>(st + ((size_t)row * ns + idx / kLnSlice) * 2) = make_float2(ssum, m2);
    }
  }
}
hipError_t launch_text_embed_emit(const int64_t* ids, const float* tok, const float* pos, void* hi, void* lo, float* st, int B,
                                  int S, int D, int vocab, int* bad_id, int dtype, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  if (D % kLnSlice || (dtype != 1 && dtype != 2)) return hipErrorInvalidValue;
  if (dtype == 1)
    hipLaunchKernelGGL(text_embed_emit_kernel<bf16_t>, dim3((B * S + 3) / 4), dim3(256), 0, s, ids, tok, pos, (unsigned short*)hi,
                       (unsigned char*)lo, st, B * S, S, D, vocab, bad_id);
  else
    hipLaunchKernelGGL(text_embed_emit_kernel<f16_t>, dim3((B * S + 3) / 4), dim3(256), 0, s, ids, tok, pos, (unsigned short*)hi,
                       (unsigned char*)lo, st, B * S, S, D, vocab, bad_id);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------
// Pooled head.  Vision: CLS row -> post_layernorm -> visual_projection (modeling_clip.py:650-651,751).
// Text: the reference applies final_layer_norm to all S rows and then picks the EOS
// row (:559-581); LayerNorm is row-wise, so picking first is exact and 77x cheaper.
// ---------------------------------------------------------------------------------
constexpr int kHeadMaxD = 2048, kHeadMaxOut = 4;  // P <= 1024
typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;

__device__ __forceinline__ float block_sum_256(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void pool_head_kernel(const float* __restrict__ x, int S, int D,
                                                        const int64_t* __restrict__ ids, int eos_id,
                                                        const float* __restrict__ ln_w, const float* __restrict__ ln_b,
                                                        float eps, const float* __restrict__ Wt, int P,
                                                        float* __restrict__ out, int normalize) {
  __shared__ float xn[kHeadMaxD];
  __shared__ float red[4];
  __shared__ int pos_s;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (tid < 64) {
    int pos = 0;
    if (ids != nullptr) {
      const int64_t* row = ids + (size_t)b * S;
      if (eos_id >= 0 && eos_id != 2) {  // first position holding eos_token_id, 0 if absent
        int best = INT_MAX;
        for (int s = tid; s < S; s += 64)
          if ((int)row[s] == eos_id) best = min(best, s);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o, 64));
        pos = best == INT_MAX ? 0 : best;
      } else {  // legacy rule: first arg-max of the ids (ids.to(int).argmax)
        int mx = INT_MIN;
        for (int s = tid; s < S; s += 64) mx = max(mx, (int)row[s]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o, 64));
        int best = INT_MAX;
        for (int s = tid; s < S; s += 64)
          if ((int)row[s] == mx) best = min(best, s);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o, 64));
        pos = best;
      }
    }
    if (tid == 0) pos_s = pos;
  }
  __syncthreads();
  const float* xr = x + ((size_t)b * S + pos_s) * D;
  float s = 0.f;
  for (int i = tid; i < D; i += 256) { const float v = xr[i]; xn[i] = v; s += v; }
  const float mean = block_sum_256(s, red) / (float)D;
  float q = 0.f;
  for (int i = tid; i < D; i += 256) { const float d = xn[i] - mean; q += d * d; }
  const float rstd = 1.0f / sqrtf(block_sum_256(q, red) / (float)D + eps);
  for (int i = tid; i < D; i += 256) xn[i] = (xn[i] - mean) * rstd * ln_w[i] + ln_b[i];
  __syncthreads();
  float o[kHeadMaxOut];
#pragma unroll
  for (int r = 0; r < kHeadMaxOut; ++r) o[r] = 0.f;
  for (int k = 0; k < D; ++k) {
    const float xv = xn[k];
    const float* wr = Wt + (size_t)k * P;
#pragma unroll
    for (int r = 0; r < kHeadMaxOut; ++r) {
      const int j = tid + r * 256;
      if (j < P) o[r] = fmaf(xv, wr[j], o[r]);
    }
  }
  float scale = 1.f;
  if (normalize) {
    float ss = 0.f;
#pragma unroll
    for (int r = 0; r < kHeadMaxOut; ++r) ss += (tid + r * 256 < P) ? o[r] * o[r] : 0.f;
    scale = 1.0f / sqrtf(block_sum_256(ss, red));
  }
#pragma unroll
  for (int r = 0; r < kHeadMaxOut; ++r) {
    const int j = tid + r * 256;
    if (j < P) out[(size_t)b * P + j] = normalize ? o[r] * scale : o[r];
  }
}

hipError_t launch_pool_head(const float* x, int S, int D, const int64_t* ids, int eos_id, const float* ln_w,
                            const float* ln_b, float eps, const float* Wt, int P, float* out, int B, int normalize,
                            hipStream_t s) {
  if (B <= 0) return hipSuccess;
  if (D > kHeadMaxD || P > kHeadMaxOut * 256) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pool_head_kernel, dim3(B), dim3(256), 0, s, x, S, D, ids, eos_id, ln_w, ln_b, eps, Wt, P, out,
                     normalize);
  return hipGetLastError();
}

// EOS row of a caption (modeling_clip.py:561-581), evaluated by one wavefront
__device__ __forceinline__ int eos_position(const int64_t* row, int S, int eos_id, int lane) {
  if (eos_id >= 0 && eos_id != 2) {  // first position holding eos_token_id, 0 if absent
    int best = INT_MAX;
    for (int s = lane; s < S; s += 64)
      if ((int)row[s] == eos_id) best = min(best, s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o, 64));
    return best == INT_MAX ? 0 : best;
  }
  int mx = INT_MIN;  // legacy rule: first arg-max of the ids
  for (int s = lane; s < S; s += 64) mx = max(mx, (int)row[s]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o, 64));
  int best = INT_MAX;
  for (int s = lane; s < S; s += 64)
    if ((int)row[s] == mx) best = min(best, s);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o, 64));
  return best;
}

// The LAST block of a tower only matters for the row that is pooled afterwards (CLS, or the caption's EOS row): one
// wavefront per sample picks that row and copies its attention output (bf16) and residual row (hi/lo planes -> fp32) into
// compact [B, D] buffers, on which out_proj / fc1 / fc2 of the last block then run (engine.hip run_last_block_pooled).
template <typename H>
__global__ __launch_bounds__(256) void pool_gather_kernel(const H* __restrict__ att, const unsigned short* __restrict__ hi,
                                                          const unsigned char* __restrict__ lo, int S, int D,
                                                          const int64_t* __restrict__ ids, int eos_id, H* __restrict__ attp,
                                                          float* __restrict__ xp, int B, const int* __restrict__ cu) {
  const int lane = threadIdx.x & 63;
  const int smp = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (smp >= B) return;
  size_t row;
  if (cu) row = (size_t)cu[smp + 1] - 1;      // packed captions end at their EOS row
  else row = (size_t)smp * S + (ids ? eos_position(ids + (size_t)smp * S, S, eos_id, lane) : 0);
  const size_t src = row * D, dst = (size_t)smp * D;
  for (int i = lane * 8; i < D; i += 512) {     // D % 8 == 0 (widths are multiples of 128)
    *reinterpret_cast<u32x4_t*>(attp + dst + i) = *reinterpret_cast<const u32x4_t*>(att + src + i);
    *reinterpret_cast<float4*>(xp + dst + i) = load4_split<H>(hi, lo, row, (unsigned)i, (unsigned)D);
    *reinterpret_cast<float4*>(xp + dst + i + 4) = load4_split<H>(hi, lo, row, (unsigned)i + 4, (unsigned)D);
  }
}
hipError_t launch_pool_gather(const void* att, const void* hi, const void* lo, int S, int D, const int64_t* ids, int eos_id,
                              void* attp, float* xp, int B, int dtype, hipStream_t s, const int* cu) {
  if (B <= 0) return hipSuccess;
  if (D % 8 || (dtype != 1 && dtype != 2)) return hipErrorInvalidValue;
  if (dtype == 1)
    hipLaunchKernelGGL(pool_gather_kernel<bf16_t>, dim3((B + 3) / 4), dim3(256), 0, s, (const bf16_t*)att, (const unsigned short*)hi,
                       (const unsigned char*)lo, S, D, ids, eos_id, (bf16_t*)attp, xp, B, cu);
  else
    hipLaunchKernelGGL(pool_gather_kernel<f16_t>, dim3((B + 3) / 4), dim3(256), 0, s, (const f16_t*)att, (const unsigned short*)hi,
                       (const unsigned char*)lo, S, D, ids, eos_id, (f16_t*)attp, xp, B, cu);
  return hipGetLastError();
}

// Packed captions: lengths (EOS position + 1), their exclusive prefix sums, the packed-row -> (sample, position) map and
// the live-row count, all on the device (nothing of it is known to the host: no synchronisation, graph-capturable).
// One workgroup of 16 waves; B and S are small (B <= max_batch, S <= 256).
__global__ __launch_bounds__(1024) void text_pack_kernel(const int64_t* __restrict__ ids, int B, int S, int eos_id,
                                                         int* __restrict__ cu, int* __restrict__ rowmap, int* __restrict__ m_dev) {
  extern __shared__ int len_s[];              // [B + 1]: lengths, then (in place) exclusive prefix sums
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  for (int b = wave; b < B; b += nw) {
    const int pos = eos_position(ids + (size_t)b * S, S, eos_id, lane);
    if (lane == 0) len_s[b] = pos + 1;
  }
  __syncthreads();
  if (threadIdx.x < 64) {                      // wave 0: chunked scan, 64 samples per step
    int carry = 0;
    for (int b0 = 0; b0 < B; b0 += 64) {
      const int v = b0 + lane < B ? len_s[b0 + lane] : 0;
      int inc = v;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
      }
      if (b0 + lane < B) len_s[b0 + lane] = carry + inc - v;
      carry += __shfl(inc, 63, 64);
    }
    if (lane == 0) { len_s[B] = carry; *m_dev = carry; }
  }
  __syncthreads();
  for (int b = threadIdx.x; b <= B; b += blockDim.x) cu[b] = len_s[b];
  for (int b = wave; b < B; b += nw) {
    const int r0 = len_s[b], n = len_s[b + 1] - r0;
    for (int t = lane; t < n; t += 64) rowmap[r0 + t] = (b << 8) | t;
  }
}
hipError_t launch_text_pack(const int64_t* ids, int B, int S, int eos_id, int* cu, int* rowmap, int* m_dev, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  if (S > 256 || B > (1 << 22)) return hipErrorInvalidValue;
  const size_t lds = (size_t)(B + 1) * sizeof(int);
  if (lds > 64 * 1024) return hipErrorInvalidValue;
  hipLaunchKernelGGL(text_pack_kernel, dim3(1), dim3(1024), lds, s, ids, B, S, eos_id, cu, rowmap, m_dev);
  return hipGetLastError();
}

template <typename H>
__global__ __launch_bounds__(256) void text_embed_emit_packed_kernel(const int64_t* __restrict__ ids, const float* __restrict__ tok,
                                                                     const float* __restrict__ pos, unsigned short* __restrict__ hi,
                                                                     unsigned char* __restrict__ lo, float* __restrict__ st,
                                                                     const int* __restrict__ rowmap, const int* __restrict__ m_dev,
                                                                     int S, int D, int vocab, int* __restrict__ bad_id) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= *m_dev) return;                  // wave-uniform
  const int bt = rowmap[row], b = bt >> 8, tpos = bt & 255;
  long long id = ids[(size_t)b * S + tpos];
  id = checked_token(id, vocab, bad_id, lane);
  const float* t = tok + (size_t)id * D;
  const float* p = pos + (size_t)tpos * D;
  const int ns = D / kLnSlice;
  for (int c0 = 0; c0 < D; c0 += 256) {
    const int idx = c0 + lane * 4;
    const bool live = idx < D;
    float4 y = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) {
      const float4 a = *reinterpret_cast<const float4*>(t + idx), c = *reinterpret_cast<const float4*>(p + idx);
      y = make_float4(a.x + c.x, a.y + c.y, a.z + c.z, a.w + c.w);
    }
    const float ssum = row16_sum((y.x + y.y) + (y.z + y.w));
    const float mj = ssum * (1.0f / kLnSlice);
    const float d0 = y.x - mj, d1 = y.y - mj, d2 = y.z - mj, d3 = y.w - mj;
    const float m2 = row16_sum((d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3));
    if (live) {
      store4_split<H>(hi, lo, (size_t)row, (unsigned)idx, (unsigned)D, y.x, y.y, y.z, y.w);
      if ((lane & 15) == 0) *reinterpret_cast<float2*>(st + ((size_t)row * ns + idx / kLnSlice) * 2) = make_float2(ssum, m2);
    }
  }
}
hipError_t launch_text_embed_emit_packed(const int64_t* ids, const float* tok, const float* pos, void* hi, void* lo, float* st,
                                         const int* rowmap, const int* m_dev, int max_rows, int S, int D, int vocab,
                                         int* bad_id, int dtype, hipStream_t s) {
  if (max_rows <= 0) return hipSuccess;
  if (D % kLnSlice || S > 256 || (dtype != 1 && dtype != 2)) return hipErrorInvalidValue;
  if (dtype == 1)
    hipLaunchKernelGGL(text_embed_emit_packed_kernel<bf16_t>, dim3((max_rows + 3) / 4), dim3(256), 0, s, ids, tok, pos,
                       (unsigned short*)hi, (unsigned char*)lo, st, rowmap, m_dev, S, D, vocab, bad_id);
  else
    hipLaunchKernelGGL(text_embed_emit_packed_kernel<f16_t>, dim3((max_rows + 3) / 4), dim3(256), 0, s, ids, tok, pos,
                       (unsigned short*)hi, (unsigned char*)lo, st, rowmap, m_dev, S, D, vocab, bad_id);
  return hipGetLastError();
}

// one wavefront per sample: pick the pooled row, LayerNorm it, write fp32 [B, D]
__global__ __launch_bounds__(256) void pool_layernorm_kernel(const float* __restrict__ x, int S, int D,
                                                             const int64_t* __restrict__ ids, int eos_id,
                                                             const float* __restrict__ g, const float* __restrict__ b,
                                                             float eps, float* __restrict__ out, int B) {
  const int lane = threadIdx.x & 63;
  const int smp = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (smp >= B) return;
  const int pos = ids ? eos_position(ids + (size_t)smp * S, S, eos_id, lane) : 0;
  const float* xr = x + ((size_t)smp * S + pos) * D;
  float4 v[kLnMaxVec];
  float s = 0.f;
#pragma unroll
  for (int it = 0; it < kLnMaxVec; ++it) {
    const int idx = it * 256 + lane * 4;
    if (idx < D) { v[it] = *reinterpret_cast<const float4*>(xr + idx); s += (v[it].x + v[it].y) + (v[it].z + v[it].w); }
  }
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int it = 0; it < kLnMaxVec; ++it) {
    const int idx = it * 256 + lane * 4;
    if (idx < D) {
      const float a = v[it].x - mean, c = v[it].y - mean, d = v[it].z - mean, e = v[it].w - mean;
      q += (a * a + c * c) + (d * d + e * e);
    }
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
  float* yr = out + (size_t)smp * D;
#pragma unroll
  for (int it = 0; it < kLnMaxVec; ++it) {
    const int idx = it * 256 + lane * 4;
    if (idx < D) {
      const float4 gg = *reinterpret_cast<const float4*>(g + idx), bb = *reinterpret_cast<const float4*>(b + idx);
      store4(yr + idx, (v[it].x - mean) * rstd * gg.x + bb.x, (v[it].y - mean) * rstd * gg.y + bb.y,
             (v[it].z - mean) * rstd * gg.z + bb.z, (v[it].w - mean) * rstd * gg.w + bb.w);
    }
  }
}
hipError_t launch_pool_layernorm(const float* x, int S, int D, const int64_t* ids, int eos_id, const float* ln_w,
                                 const float* ln_b, float eps, float* out, int B, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  if (D % 4 || D > kLnMaxVec * 256) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pool_layernorm_kernel, dim3((B + 3) / 4), dim3(256), 0, s, x, S, D, ids, eos_id, ln_w, ln_b, eps, out, B);
  return hipGetLastError();
}

// x / sqrt(sum x^2), no epsilon (modeling_clip.py:57-65; plip.py:75)
__global__ __launch_bounds__(256) void l2_normalize_kernel(float* __restrict__ x, int N, int D) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  float* xr = x + (size_t)row * D;
  float ss = 0.f;
  for (int i = lane; i < D; i += 64) ss += xr[i] * xr[i];
  const float scale = 1.0f / sqrtf(wave_sum(ss));
  for (int i = lane; i < D; i += 64) xr[i] *= scale;
}
hipError_t launch_l2_normalize(float* x, int N, int D, hipStream_t s) {
  if (N <= 0) return hipSuccess;
  hipLaunchKernelGGL(l2_normalize_kernel, dim3((N + 3) / 4), dim3(256), 0, s, x, N, D);
  return hipGetLastError();
}

// Occupies ONE compute unit for `ticks` of the constant-rate wall clock (s_memrealtime) and touches no memory: two of these on two
// streams finish in the time of one when the streams sit on different hardware queues, and one after the other when they share a
// queue -- what plipmi_streams_overlap measures.  Bounded (about a second) whatever the clock does.
__global__ __launch_bounds__(64) void occupy_kernel(unsigned long long ticks) {
  const unsigned long long t0 = wall_clock64();
  for (int i = 0; i < (1 << 22) && wall_clock64() - t0 < ticks; ++i) __builtin_amdgcn_s_sleep(8);
}
hipError_t launch_occupy(unsigned long long ticks, hipStream_t s) {
  hipLaunchKernelGGL(occupy_kernel, dim3(1), dim3(64), 0, s, ticks);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------
// Logits: logits_per_image = scale * img @ txt^T (modeling_clip.py:814-817), fp32 FMA.
// 64x64 tile per 256-thread block, 4x4 outputs per thread, K staged through LDS in
// chunks of 16.  Any Ni / Nt (zero-shot uses Nt = number of class prompts).
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void logits_kernel(const float* __restrict__ A, int Ni, const float* __restrict__ Bm,
                                                     int Nt, int D, float scale, float* __restrict__ lpi,
                                                     float* __restrict__ lpt) {
  __shared__ float As[16][68];
  __shared__ float Bs[16][68];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int i0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
  float acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[a][c] = 0.f;
  const int lr = tid >> 2, lk = (tid & 3) * 4;  // each thread stages 4 consecutive k of one row
  for (int k0 = 0; k0 < D; k0 += 16) {
    float av[4] = {0.f, 0.f, 0.f, 0.f}, bv[4] = {0.f, 0.f, 0.f, 0.f};
    if (i0 + lr < Ni)
#pragma unroll
      for (int e = 0; e < 4; ++e) if (k0 + lk + e < D) av[e] = A[(size_t)(i0 + lr) * D + k0 + lk + e];
    if (j0 + lr < Nt)
#pragma unroll
      for (int e = 0; e < 4; ++e) if (k0 + lk + e < D) bv[e] = Bm[(size_t)(j0 + lr) * D + k0 + lk + e];
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) { As[lk + e][lr] = av[e]; Bs[lk + e][lr] = bv[e]; }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      float a[4], b[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) { a[e] = As[k][ty * 4 + e]; b[e] = Bs[k][tx * 4 + e]; }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = fmaf(a[r], b[c], acc[r][c]);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + ty * 4 + r;
    if (i >= Ni) continue;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = j0 + tx * 4 + c;
      if (j >= Nt) continue;
      const float v = acc[r][c] * scale;
      lpi[(size_t)i * Nt + j] = v;
      if (lpt) lpt[(size_t)j * Ni + i] = v;
    }
  }
}

// first arg-max of each row (np.argmax / torch.argmax semantics for ties)
__global__ __launch_bounds__(256) void row_argmax_kernel(const float* __restrict__ x, int N, int M,
                                                         int32_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const float* xr = x + (size_t)row * M;
  float best = -INFINITY;
  int bi = INT_MAX;
  for (int j = lane; j < M; j += 64) {
    const float v = xr[j];
    if (v > best || bi == INT_MAX) { best = v; bi = j; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (oi != INT_MAX && (bi == INT_MAX || ov > best || (ov == best && oi < bi))) { best = ov; bi = oi; }
  }
  if (lane == 0) out[row] = bi == INT_MAX ? 0 : bi;
}

hipError_t launch_logits(const float* img, int Ni, const float* txt, int Nt, int D, float scale, float* lpi,
                         float* lpt, int32_t* argmax, hipStream_t s) {
  if (Ni <= 0 || Nt <= 0) return hipSuccess;
  hipLaunchKernelGGL(logits_kernel, dim3((Nt + 63) / 64, (Ni + 63) / 64), dim3(256), 0, s, img, Ni, txt, Nt, D, scale,
                     lpi, lpt);
  if (argmax) hipLaunchKernelGGL(row_argmax_kernel, dim3((Ni + 3) / 4), dim3(256), 0, s, lpi, Ni, Nt, argmax);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------
// top-k per row, descending, ties -> lower index (replaces argsort()[:, -k:][:, ::-1],
// plip.py:84; retrieval.py:17).  k selection passes, each a block-wide arg-max over
// the keys strictly after the previous pick in (value desc, index asc) order.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void topk_kernel(const float* __restrict__ x, int M, int k, int64_t* __restrict__ out) {
  __shared__ float rv[4];
  __shared__ int ri[4];
  const float* xr = x + (size_t)blockIdx.x * M;
  float pv = INFINITY;
  int pi = -1;
  for (int t = 0; t < k; ++t) {
    float best = -INFINITY;
    int bi = INT_MAX;
    for (int j = threadIdx.x; j < M; j += 256) {
      float v = xr[j];
      if (!(v == v)) v = -INFINITY;  // NaN sorts last
      const bool after = (v < pv) || (v == pv && j > pi);
      if (after && (v > best || (v == best && j < bi))) { best = v; bi = j; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { rv[threadIdx.x >> 6] = best; ri[threadIdx.x >> 6] = bi; }
    __syncthreads();
    best = rv[0]; bi = ri[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
      if (rv[w] > best || (rv[w] == best && ri[w] < bi)) { best = rv[w]; bi = ri[w]; }
    if (threadIdx.x == 0) out[(size_t)blockIdx.x * k + t] = bi == INT_MAX ? -1 : bi;
    pv = best; pi = bi;
  }
}
hipError_t launch_topk(const float* scores, int N, int M, int k, int64_t* idx, hipStream_t s) {
  if (N <= 0 || k <= 0) return hipSuccess;
  if (k > M) return hipErrorInvalidValue;
  hipLaunchKernelGGL(topk_kernel, dim3(N), dim3(256), 0, s, scores, M, k, idx);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------
// Projection head GEMM: out[B, P] = pooled[B, D] . W[P, D]^T in exact fp32 (modeling_clip.py:674-675,713,751).
// 100 MFLOP on a 256 x 512 output: with the big-tile GEMM this was 8 workgroups walking 24 K tiles one after the
// other (46 us, latency-bound, at the tail of each tower).  Here one workgroup owns a 32 x 32 output tile, its four
// waves split K four ways (fp32 32x32x2 MFMA, operands straight from L2 as float4 per lane -- the k index inside an
// MFMA may be permuted freely as long as both operands share the permutation), and the partial tiles are added
// through LDS in a fixed order (deterministic, independent of the batch size).
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void head_gemm_kernel(const float* __restrict__ A, const float* __restrict__ W,
                                                        float* __restrict__ C, int M, int N, int K, float scale) {
  __shared__ __attribute__((aligned(16))) float part[4][16][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lrow = lane & 31, lgrp = lane >> 5;
  const int n0 = blockIdx.x * 32, m0 = blockIdx.y * 32;
  const int ar = m0 + lrow < M ? m0 + lrow : M - 1;
  const int kq = K / 4;  // K % 32 == 0 -> a multiple of 8
  const float* ap = A + (size_t)ar * K + wave * kq + 4 * lgrp;
  const float* wp = W + (size_t)(n0 + lrow) * K + wave * kq + 4 * lgrp;
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  for (int kk = 0; kk < kq; kk += 8) {
    const float4 a = *reinterpret_cast<const float4*>(ap + kk);
    const float4 w = *reinterpret_cast<const float4*>(wp + kk);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.x, a.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.y, a.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.z, a.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.w, a.w, acc, 0, 0, 0);
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) part[wave][e][lane] = acc[e];
  __syncthreads();
  // wave q finishes accumulator quad q: C[m0 + lrow][n0 + 8q + 4*lgrp + e]
  float4 o;
  float* op = &o.x;
#pragma unroll
  for (int e = 0; e < 4; ++e)
    op[e] = scale * (((part[0][4 * wave + e][lane] + part[1][4 * wave + e][lane]) + part[2][4 * wave + e][lane]) + part[3][4 * wave + e][lane]);
  if (m0 + lrow < M) *reinterpret_cast<float4*>(C + (size_t)(m0 + lrow) * N + n0 + 8 * wave + 4 * lgrp) = o;
}
hipError_t launch_head_gemm(const float* A, const float* W, float* C, int M, int N, int K, hipStream_t s, float scale) {
  if (M <= 0) return hipSuccess;
  if (N % 32 || K % 32) return hipErrorInvalidValue;
  hipLaunchKernelGGL(head_gemm_kernel, dim3(N / 32, (M + 31) / 32), dim3(256), 0, s, A, W, C, M, N, K, scale);
  return hipGetLastError();
}
hipError_t launch_row_argmax(const float* x, int N, int M, int32_t* out, hipStream_t s) {
  if (N <= 0) return hipSuccess;
  hipLaunchKernelGGL(row_argmax_kernel, dim3((N + 3) / 4), dim3(256), 0, s, x, N, M, out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------
// Streaming top-k (fused similarity + top-k head, plipmi_similarity_topk).
// The score matrix is produced panel by panel ([rows, <=8192] fp32, never the full [Nq, Ns]); this kernel folds
// one panel into each row's running top-k list.  One wavefront per query row; the list (k <= 1024 entries,
// descending, ties: lower global index first) lives in LDS.  A column only costs an LDS insertion if it beats
// the row's current k-th best, which after the first panel is rare (k ln(N/k) insertions per row in total), so
// the scan runs at streaming rate: 16 B per lane per step, one ballot per component.
// Order: (v, i) is better than (w, j) iff v > w or (v == w and i < j); NaN scores count as -inf.
// ---------------------------------------------------------------------------------
__device__ __forceinline__ bool topk_better(float v, long long i, float w, long long j) {
  return v > w || (v == w && i < j);
}

__global__ __launch_bounds__(256) void topk_merge_kernel(const float* __restrict__ scores, size_t ld, int rows,
                                                         int ncols, long long col0, int k, float* __restrict__ vals,
                                                         long long* __restrict__ idx) {
  extern __shared__ __attribute__((aligned(16))) char topk_smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + wave;
  if (row >= rows) return;  // whole wave; no workgroup barrier below
  long long* si = reinterpret_cast<long long*>(topk_smem) + (size_t)wave * k;
  float* sv = reinterpret_cast<float*>(topk_smem + (size_t)4 * k * sizeof(long long)) + (size_t)wave * k;
  float* gv = vals + (size_t)row * k;
  long long* gi = idx + (size_t)row * k;
  for (int e = lane; e < k; e += 64) { sv[e] = gv[e]; si[e] = gi[e]; }
  float tv = sv[k - 1];
  long long ti = si[k - 1];
  const float* sr = scores + (size_t)row * ld;
  for (int j0 = 0; j0 < ncols; j0 += 256) {
    const int j = j0 + lane * 4;
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j + 3 < ncols) q = *reinterpret_cast<const float4*>(sr + j);
    else {
      if (j < ncols) q.x = sr[j];
      if (j + 1 < ncols) q.y = sr[j + 1];
      if (j + 2 < ncols) q.z = sr[j + 2];
    }
    const float comp[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float v = comp[c];
      if (!(v == v)) v = -INFINITY;
      const long long g = col0 + j + c;
      unsigned long long mask = __ballot(j + c < ncols && topk_better(v, g, tv, ti));
      while (mask) {
        const int l = __builtin_ctzll(mask);
        mask &= mask - 1;
        const float vv = __shfl(v, l, 64);
        const long long ii = __shfl(g, l, 64);
        if (!topk_better(vv, ii, tv, ti)) continue;  // the k-th best moved since the ballot (wave-uniform)
        int pos = 0;
        for (int e0 = 0; e0 < k; e0 += 64) {
          const int e = e0 + lane;
          pos += __popcll(__ballot(e < k && topk_better(sv[e], si[e], vv, ii)));
        }
        // entries [pos, k-2] move down one slot, highest chunk first; inside a chunk every lane reads before any writes
        for (int e0 = ((k - 1) >> 6) << 6; e0 >= 0; e0 -= 64) {
          const int e = e0 + lane;
          const bool mv = e > pos && e < k;
          const float mvv = mv ? sv[e - 1] : 0.f;
          const long long mvi = mv ? si[e - 1] : 0;
          __builtin_amdgcn_wave_barrier();
          if (mv) { sv[e] = mvv; si[e] = mvi; }
          __builtin_amdgcn_wave_barrier();
        }
        if (lane == 0) { sv[pos] = vv; si[pos] = ii; }
        __builtin_amdgcn_wave_barrier();
        tv = sv[k - 1];
        ti = si[k - 1];
      }
    }
  }
  for (int e = lane; e < k; e += 64) { gv[e] = sv[e]; gi[e] = si[e]; }
}

__global__ void topk_init_kernel(float* __restrict__ vals, long long* __restrict__ idx, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    vals[i] = -INFINITY;
    idx[i] = LLONG_MAX;  // an empty slot loses every tie
  }
}
// empty slots (fewer than k finite candidates cannot happen for k <= Ns, but keep the contract of launch_topk) -> -1
__global__ void topk_finish_kernel(long long* __restrict__ idx, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    if (idx[i] == LLONG_MAX) idx[i] = -1;
}

hipError_t launch_topk_init(float* vals, int64_t* idx, size_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  const int grid = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
  hipLaunchKernelGGL(topk_init_kernel, dim3(grid), dim3(256), 0, s, vals, reinterpret_cast<long long*>(idx), n);
  return hipGetLastError();
}
hipError_t launch_topk_finish(int64_t* idx, size_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  const int grid = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
  hipLaunchKernelGGL(topk_finish_kernel, dim3(grid), dim3(256), 0, s, reinterpret_cast<long long*>(idx), n);
  return hipGetLastError();
}
hipError_t launch_topk_merge(const float* scores, size_t ld, int rows, int ncols, int64_t col0, int k, float* vals,
                             int64_t* idx, hipStream_t s) {
  if (rows <= 0 || ncols <= 0) return hipSuccess;
  if (k <= 0 || k > kTopkMaxK || (ld & 3)) return hipErrorInvalidValue;
  const size_t smem = (size_t)4 * k * (sizeof(long long) + sizeof(float));
  hipLaunchKernelGGL(topk_merge_kernel, dim3((rows + 3) / 4), dim3(256), smem, s, scores, ld, rows, ncols,
                     (long long)col0, k, vals, reinterpret_cast<long long*>(idx));
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------
// Resize (8-bit bicubic, Pillow's integer arithmetic) + centre crop on uint8 HWC images: the step in front of
// plipmi_encode_image_u8 (transform.py:45-52 / CLIPImageProcessor resize + center_crop).  The coefficient tables
// come from the host (plip_amd/preprocess.py, float64 exactly as Pillow builds them); both passes are int32
// accumulations from 2^21 with an arithmetic shift by 22 and a clamp, horizontal first, uint8 in between --
// bit-identical to Image.resize(BICUBIC).crop(...).  Only the crop window is computed.
// ---------------------------------------------------------------------------------
__device__ __forceinline__ uint8_t clip8_fixed(int acc) {
  const int v = acc >> 22;
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}
__global__ __launch_bounds__(256) void resize_h_kernel(const uint8_t* __restrict__ src, int H, int W,
                                                       const int* __restrict__ xb, const int* __restrict__ xk, int ks,
                                                       int left, int r0, int R, int n, uint8_t* __restrict__ tmp,
                                                       size_t total) {
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int x = (int)(idx % n);
    const size_t t = idx / n;
    const int y = (int)(t % R);
    const size_t b = t / R;
    const uint8_t* row = src + ((b * H + r0 + y) * (size_t)W) * 3;
    uint8_t* o = tmp + idx * 3;
    if (xb == nullptr) {  // width already right: this pass is only the crop
      const uint8_t* px = row + (size_t)(left + x) * 3;
      o[0] = px[0]; o[1] = px[1]; o[2] = px[2];
      continue;
    }
    const int x0 = xb[2 * x], cnt = xb[2 * x + 1];
    const int* k = xk + (size_t)x * ks;
    int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
    const uint8_t* px = row + (size_t)x0 * 3;
    for (int i = 0; i < cnt; ++i) {
      const int w = k[i];
      a0 += px[3 * i + 0] * w; a1 += px[3 * i + 1] * w; a2 += px[3 * i + 2] * w;
    }
    o[0] = clip8_fixed(a0); o[1] = clip8_fixed(a1); o[2] = clip8_fixed(a2);
  }
}
__global__ __launch_bounds__(256) void resize_v_kernel(const uint8_t* __restrict__ tmp, int R, int n,
                                                       const int* __restrict__ yb, const int* __restrict__ yk, int ks,
                                                       int r0, int top, uint8_t* __restrict__ dst, size_t total) {
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int xc = (int)(idx % (n * 3));  // (x, channel) flattened: rows of tmp are n*3 contiguous bytes
    const size_t t = idx / (n * 3);
    const int y = (int)(t % n);
    const size_t b = t / n;
    const uint8_t* img = tmp + b * (size_t)R * n * 3;
    if (yb == nullptr) {
      dst[idx] = img[(size_t)(top + y - r0) * n * 3 + xc];
      continue;
    }
    const int y0 = yb[2 * y] - r0, cnt = yb[2 * y + 1];
    const int* k = yk + (size_t)y * ks;
    int a = 1 << 21;
    for (int i = 0; i < cnt; ++i) a += img[(size_t)(y0 + i) * n * 3 + xc] * k[i];
    dst[idx] = clip8_fixed(a);
  }
}
hipError_t launch_resize_crop_u8(const uint8_t* src, int B, int H, int W, int n, const int* xb, const int* xk, int xks,
                                 int left, const int* yb, const int* yk, int yks, int top, int r0, int R,
                                 uint8_t* tmp, uint8_t* dst, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  const size_t th = (size_t)B * R * n, tv = (size_t)B * n * n * 3;
  const int gh = (int)((th + 255) / 256 < 65536 ? (th + 255) / 256 : 65536);
  const int gv = (int)((tv + 255) / 256 < 65536 ? (tv + 255) / 256 : 65536);
  hipLaunchKernelGGL(resize_h_kernel, dim3(gh), dim3(256), 0, s, src, H, W, xb, xk, xks, left, r0, R, n, tmp, th);
  hipLaunchKernelGGL(resize_v_kernel, dim3(gv), dim3(256), 0, s, tmp, R, n, yb, yk, yks, r0, top, dst, tv);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------
// weight packing (plipmi_create)
// ---------------------------------------------------------------------------------
template <typename T>
__global__ void convert_kernel(const float* __restrict__ src, T* __restrict__ dst, int rows, int cols, int dst_ld,
                               float scale) {
  const size_t n = (size_t)rows * dst_ld;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / dst_ld), c = (int)(i - (size_t)r * dst_ld);
    dst[i] = from_f32<T>(c < cols ? src[(size_t)r * cols + c] * scale : 0.f);
  }
}
hipError_t launch_convert(const float* src, void* dst, int dst_dtype, int rows, int cols, int dst_ld, float scale,
                          hipStream_t s) {
  const size_t n = (size_t)rows * dst_ld;
  if (n == 0) return hipSuccess;
  const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  if (dst_dtype == 1)
    hipLaunchKernelGGL(convert_kernel<bf16_t>, dim3(grid), dim3(256), 0, s, src, (bf16_t*)dst, rows, cols, dst_ld, scale);
  else if (dst_dtype == 2)
    hipLaunchKernelGGL(convert_kernel<f16_t>, dim3(grid), dim3(256), 0, s, src, (f16_t*)dst, rows, cols, dst_ld, scale);
  else
    hipLaunchKernelGGL(convert_kernel<float>, dim3(grid), dim3(256), 0, s, src, (float*)dst, rows, cols, dst_ld, scale);
  return hipGetLastError();
}

__global__ void transpose_kernel(const float* __restrict__ src, float* __restrict__ dst, int rows, int cols) {
  __shared__ float t[32][33];
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  for (int i = threadIdx.y; i < 32; i += 8) {
    const int r = r0 + i, c = c0 + threadIdx.x;
    t[i][threadIdx.x] = (r < rows && c < cols) ? src[(size_t)r * cols + c] : 0.f;
  }
  __syncthreads();
  for (int i = threadIdx.y; i < 32; i += 8) {
    const int c = c0 + i, r = r0 + threadIdx.x;
    if (r < rows && c < cols) dst[(size_t)c * rows + r] = t[threadIdx.x][i];
  }
}
hipError_t launch_transpose(const float* src, float* dst, int rows, int cols, hipStream_t s) {
  hipLaunchKernelGGL(transpose_kernel, dim3((cols + 31) / 32, (rows + 31) / 32), dim3(32, 8), 0, s, src, dst, rows, cols);
  return hipGetLastError();
}

__global__ void scale_copy_kernel(const float* __restrict__ src, float* __restrict__ dst, int n, float scale) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) dst[i] = src[i] * scale;
}
hipError_t launch_scale_copy(const float* src, float* dst, int n, float scale, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(scale_copy_kernel, dim3((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024), dim3(256), 0, s, src, dst,
                     n, scale);
  return hipGetLastError();
}

// rows[b] = the row of sample b that the heads pool (0 when ids == nullptr, else the caption's EOS row): one wavefront per sample
__global__ __launch_bounds__(256) void pooled_row_index_kernel(const int64_t* __restrict__ ids, int S, int eos_id, int* __restrict__ rows,
                                                               int B) {
  const int lane = threadIdx.x & 63;
  const int smp = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (smp >= B) return;
  const int pos = ids ? eos_position(ids + (size_t)smp * S, S, eos_id, lane) : 0;
  if (lane == 0) rows[smp] = pos;
}
hipError_t launch_pooled_row_index(const int64_t* ids, int S, int eos_id, int* rows, int B, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  if (S <= 0 || !rows) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pooled_row_index_kernel, dim3((B + 3) / 4), dim3(256), 0, s, ids, S, eos_id, rows, B);
  return hipGetLastError();
}

}  // namespace plipmi
