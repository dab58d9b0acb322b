// tower_kernels.hip -- the HBM-bound kernels a tower forward (or one of its tap entries) launches around the GEMMs and the
// attention: the LayerNorm family, the residual planes, patch unfold, embeddings, caption packing, the pooled rows and the
// projection head.  (After the embeddings: head_kernels.hip; once per handle: setup_kernels.hip.)  All are wavefront(64)-shaped: one
// wave per row for row reductions (shuffle/DPP reductions, no LDS), 16-byte accesses per lane, fp32 statistics.
#include <limits.h>

#include "dispatch.h"
#include "kernels.h"

namespace plipmi {

// ---------------------------------------------------------------------------------
// LayerNorm (nn.LayerNorm, biased variance; modeling_clip.py:358,360,559,605,608)
// ---------------------------------------------------------------------------------
constexpr int kLnMaxVec = 8;  // float4 per lane -> D <= 2048

// The arithmetic of the two-pass row LayerNorm, one lane's float4 at a time, for the four kernels that do it (but see the store
// loop of layernorm_fixed_kernel).  The loops stay in the kernels: a register array handed to a helper compiles differently.
__device__ __forceinline__ float ln_sum4(float4 v) { return (v.x + v.y) + (v.z + v.w); }
__device__ __forceinline__ float ln_sq4(float4 v, float mean) {   // centred sum of squares
  const float a = v.x - mean, c = v.y - mean, d = v.z - mean, e = v.w - mean;
  return (a * a + c * c) + (d * d + e * e);
}
__device__ __forceinline__ float ln_rstd(float sq, int D, float eps) { return 1.0f / sqrtf(sq / (float)D + eps); }
__device__ __forceinline__ float4 ln_apply4(float4 v, float mean, float rstd, float4 g, float4 b) {
  return make_float4((v.x - mean) * rstd * g.x + b.x, (v.y - mean) * rstd * g.y + b.y, (v.z - mean) * rstd * g.z + b.z,
                     (v.w - mean) * rstd * g.w + b.w);
}

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
    if (idx < D) { v[it] = *reinterpret_cast<const float4*>(xr + idx); s += ln_sum4(v[it]); }
  }
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int it = 0; it < kLnMaxVec; ++it) {
    const int idx = it * 256 + lane * 4;
    if (idx < D) q += ln_sq4(v[it], mean);
  }
  const float rstd = ln_rstd(wave_sum(q), D, eps);
  TOut* yr = y + (size_t)row * D;
#pragma unroll
  for (int it = 0; it < kLnMaxVec; ++it) {
    const int idx = it * 256 + lane * 4;
    if (idx < D) {
      const float4 gg = *reinterpret_cast<const float4*>(g + idx), bb = *reinterpret_cast<const float4*>(b + idx);
      const float4 y = ln_apply4(v[it], mean, rstd, gg, bb);
      store4(yr + idx, y.x, y.y, y.z, y.w);
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
    for (int it = 0; it < NV; ++it) s += ln_sum4(v[r][it]);
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int it = 0; it < NV; ++it) q += ln_sq4(v[r][it], mean);
    const float rstd = ln_rstd(wave_sum(q), D, eps);
    if (row0 + r < rows) {
      TOut* yr = y + (size_t)(row0 + r) * D;
#pragma unroll
      for (int it = 0; it < NV; ++it)   // ln_apply4's expression, written out ON PURPOSE: through the helper all six instantiations reorder
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
//   * the weights' side of the fold: setup_kernels.hip fold_ln_kernel.
// ---------------------------------------------------------------------------------
// One 256-column chunk of a row of the split residual stream, the one source of it for the three emit kernels: lane's four values y
// (columns idx .., zero when !live, i.e. idx >= D) go to the hi / lo planes, each 64-column slice (16 lanes) stores its {sum, centred
// M2} partial to st [rows, ns = D / kLnSlice, 2].  Every lane of the wave calls it (DPP row reductions).  Plain pointers, and ns
// from the caller: with __restrict__ parameters or the division in here the callers compile differently.
template <typename H>
__device__ __forceinline__ void emit_chunk(unsigned short* hi, unsigned char* lo, float* st, int row, int ns, int idx, int D, bool live,
                                           int lane, float4 y) {
  const float ssum = row16_sum((y.x + y.y) + (y.z + y.w));
  const float mj = ssum * (1.0f / kLnSlice);
  const float d0 = y.x - mj, d1 = y.y - mj, d2 = y.z - mj, d3 = y.w - mj;
  const float m2 = row16_sum((d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3));
  if (live) {
    store4_split<H>(hi, lo, (size_t)row, (unsigned)idx, (unsigned)D, y.x, y.y, y.z, y.w);
    if ((lane & 15) == 0) *reinterpret_cast<float2*>(st + ((size_t)row * ns + idx / kLnSlice) * 2) = make_float2(ssum, m2);
  }
}

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
    s += ln_sum4(v[it]);
  }
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int it = 0; it < kLnMaxVec; ++it) {
    const int idx = it * 256 + lane * 4;
    if (idx < D) q += ln_sq4(v[it], mean);
  }
  const float rstd = ln_rstd(wave_sum(q), D, eps);
  const int ns = D / kLnSlice;
#pragma unroll
  for (int it = 0; it < kLnMaxVec; ++it) {
    const int idx = it * 256 + lane * 4;       // 16 lanes = one 64-column slice (D % 64 == 0)
    if (it * 256 >= D) break;                    // wave-uniform: every lane runs the DPP reductions of a live chunk
    const bool live = idx < D;
    float4 y = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) {
      const float4 gg = *reinterpret_cast<const float4*>(g + idx), bb = *reinterpret_cast<const float4*>(b + idx);
      y = ln_apply4(v[it], mean, rstd, gg, bb);
    }
    emit_chunk<H>(hi, lo, st, row, ns, idx, D, live, lane, y);
  }
}
hipError_t launch_layernorm_emit(const float* x, const float* g, const float* b, void* hi, void* lo, float* st, int rows, int D,
                                 float eps, int dtype, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (D % kLnSlice || D > kLnMaxVec * 256 || (dtype != 1 && dtype != 2)) return hipErrorInvalidValue;
  with_half(dtype, [&](auto tag) {
    hipLaunchKernelGGL(layernorm_emit_kernel<decltype(tag)>, dim3((rows + 3) / 4), dim3(256), 0, s, x, g, b, (unsigned short*)hi,
                       (unsigned char*)lo, st, rows, D, eps);
  });
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
  with_half(dtype, [&](auto tag) {
    hipLaunchKernelGGL(join_planes_kernel<decltype(tag)>, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, s, (const unsigned short*)hi,
                       (const unsigned char*)lo, x, n / 4, (unsigned)D);
  });
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

hipError_t launch_layernorm(const float* x, size_t xs, const float* g, const float* b, void* y, int y_dtype, int rows,
                            int D, float eps, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (D % 4 || D > kLnMaxVec * 256) return hipErrorInvalidValue;
  if (y_dtype != 0 && (D == 512 || D == 768 || D == 1024)) {  // one kernel for every batch size: batch invariance is bitwise
    constexpr int RPW = 2;
    const dim3 grid((rows + 4 * RPW - 1) / (4 * RPW)), block(256);
    with_half(y_dtype, [&](auto tag) {
      using H = decltype(tag);
      if (D == 512) hipLaunchKernelGGL((layernorm_fixed_kernel<H, 2, RPW>), grid, block, 0, s, x, xs, g, b, (H*)y, rows, eps);
      else if (D == 768) hipLaunchKernelGGL((layernorm_fixed_kernel<H, 3, RPW>), grid, block, 0, s, x, xs, g, b, (H*)y, rows, eps);
      else hipLaunchKernelGGL((layernorm_fixed_kernel<H, 4, RPW>), grid, block, 0, s, x, xs, g, b, (H*)y, rows, eps);
    });
    return hipGetLastError();
  }
  const dim3 grid((rows + 3) / 4), block(256);
  with_dtype(y_dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(layernorm_kernel<T>, grid, block, 0, s, x, xs, g, b, (T*)y, rows, D, eps);
  });
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
  with_dtype(out_dtype, [&](auto tag) {
    using T = decltype(tag);
    if (vec) hipLaunchKernelGGL((unfold_kernel<T, true>), grid, block, 0, s, pixels, (T*)out, H, W, patch, K, Kpad);
    else hipLaunchKernelGGL((unfold_kernel<T, false>), grid, block, 0, s, pixels, (T*)out, H, W, patch, K, Kpad);
  });
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
  with_dtype(out_dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(unfold_u8_kernel<T>, grid, block, 0, s, tiles, (T*)out, H, W, patch, K, Kpad);
  });
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
  const long long id = checked_token(ids[row], vocab, bad_id, threadIdx.x);
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

// one row of token + position embedding as split planes + statistics partials (one wavefront; t / p = the row's table rows)
template <typename H>
__device__ __forceinline__ void embed_emit_row(const float* t, const float* p, unsigned short* hi, unsigned char* lo, float* st, int row,
                                               int D, int lane) {
  const int ns = D / kLnSlice;
  for (int c0 = 0; c0 < D; c0 += 256) {          // wave-uniform trip count
    const int idx = c0 + lane * 4;
    const bool live = idx < D;
    float4 y = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) {
      const float4 a = *reinterpret_cast<const float4*>(t + idx), b = *reinterpret_cast<const float4*>(p + idx);
      y = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
    }
    emit_chunk<H>(hi, lo, st, row, ns, idx, D, live, lane, y);
  }
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
  const long long id = checked_token(ids[row], vocab, bad_id, lane);
  const float* t = tok + (size_t)id * D;
  const float* p = pos + (size_t)(row % S) * D;
  embed_emit_row<H>(t, p, hi, lo, st, row, D, lane);
}
hipError_t launch_text_embed_emit(const int64_t* ids, const float* tok, const float* pos, void* hi, void* lo, float* st, int B,
                                  int S, int D, int vocab, int* bad_id, int dtype, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  if (D % kLnSlice || (dtype != 1 && dtype != 2)) return hipErrorInvalidValue;
  with_half(dtype, [&](auto tag) {
    hipLaunchKernelGGL(text_embed_emit_kernel<decltype(tag)>, dim3((B * S + 3) / 4), dim3(256), 0, s, ids, tok, pos, (unsigned short*)hi,
                       (unsigned char*)lo, st, B * S, S, D, vocab, bad_id);
  });
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------
// Pooled head.  Vision: CLS row -> post_layernorm -> visual_projection (modeling_clip.py:650-651,751).
// Text: the reference applies final_layer_norm to all S rows and then picks the EOS
// row (:559-581); LayerNorm is row-wise, so picking first is exact and 77x cheaper.
// ---------------------------------------------------------------------------------

// EOS row of a caption (modeling_clip.py:561-581), evaluated by one wavefront: the one statement of the rule for pool_head,
// pool_gather, text_pack, pool_layernorm and pooled_row_index
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
    const int pos = ids != nullptr ? eos_position(ids + (size_t)b * S, S, eos_id, tid) : 0;
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
  with_half(dtype, [&](auto tag) {
    using H = decltype(tag);
    hipLaunchKernelGGL(pool_gather_kernel<H>, dim3((B + 3) / 4), dim3(256), 0, s, (const H*)att, (const unsigned short*)hi,
                       (const unsigned char*)lo, S, D, ids, eos_id, (H*)attp, xp, B, cu);
  });
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
  const long long id = checked_token(ids[(size_t)b * S + tpos], vocab, bad_id, lane);
  const float* t = tok + (size_t)id * D;
  const float* p = pos + (size_t)tpos * D;
  embed_emit_row<H>(t, p, hi, lo, st, row, D, lane);
}
hipError_t launch_text_embed_emit_packed(const int64_t* ids, const float* tok, const float* pos, void* hi, void* lo, float* st,
                                         const int* rowmap, const int* m_dev, int max_rows, int S, int D, int vocab,
                                         int* bad_id, int dtype, hipStream_t s) {
  if (max_rows <= 0) return hipSuccess;
  if (D % kLnSlice || S > 256 || (dtype != 1 && dtype != 2)) return hipErrorInvalidValue;
  with_half(dtype, [&](auto tag) {
    hipLaunchKernelGGL(text_embed_emit_packed_kernel<decltype(tag)>, dim3((max_rows + 3) / 4), dim3(256), 0, s, ids, tok, pos,
                       (unsigned short*)hi, (unsigned char*)lo, st, rowmap, m_dev, S, D, vocab, bad_id);
  });
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
    if (idx < D) { v[it] = *reinterpret_cast<const float4*>(xr + idx); s += ln_sum4(v[it]); }
  }
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int it = 0; it < kLnMaxVec; ++it) {
    const int idx = it * 256 + lane * 4;
    if (idx < D) q += ln_sq4(v[it], mean);
  }
  const float rstd = ln_rstd(wave_sum(q), D, eps);
  float* yr = out + (size_t)smp * D;
#pragma unroll
  for (int it = 0; it < kLnMaxVec; ++it) {
    const int idx = it * 256 + lane * 4;
    if (idx < D) {
      const float4 gg = *reinterpret_cast<const float4*>(g + idx), bb = *reinterpret_cast<const float4*>(b + idx);
      const float4 y = ln_apply4(v[it], mean, rstd, gg, bb);
      store4(yr + idx, y.x, y.y, y.z, y.w);
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
