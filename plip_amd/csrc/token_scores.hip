// token_scores.hip -- the last launch of plipmi_encode_token_similarity (include/plipmi.h): per token row, the cosine of its projected
// embedding with every text row, scaled, optionally softmaxed over the text rows.  All fp32.
//
//   out[m, c] = scale * <E[m] / |E[m]|, T[c] / |T[c]|>            E [M, P] token embeddings, T [C, P] text embeddings (any norm)
//   softmax:   out[m, :] = softmax_c of those values, max-subtracted
//
//   token_scores_kernel   one workgroup of 256 lanes owns 16 token rows: 16 lanes per row (a DPP row), lane l of a row holds the 16-byte
//                         pieces l, l + 16, l + 32, .. of E[m] in registers for the whole kernel (NV of them: P <= 64 NV).  The text rows
//                         pass through LDS sixteen at a time; each of the workgroup's 16 lane groups first forms one staged text row's
//                         1 / |T[c]| (the prologue of the chunk: no scratch, no second launch), then every group takes the 16 dot
//                         products of its token row against the chunk -- one ds_read_b128 per four fmaf, the four groups of a wave read
//                         the same addresses (a broadcast), the 16 lanes of a group 256 contiguous bytes.  Lane c & 15 of the group keeps
//                         score c in register c >> 4, so scale, max, exp, sum and the store touch 16 lanes x 4 registers and the store of
//                         a row is up to four runs of 64 contiguous bytes.
// Sums run in a fixed order -- per lane over its pieces in ascending order (one fmaf chain x, y, z, w per piece), then the DPP butterfly
// of row16_sum -- that depends on P alone: a row's output bits are the same whatever M is and wherever the row sits.  No epsilon: a zero
// row of E or T gives non-finite scores (as launch_l2_normalize does).
// All stores are ordinary vector stores; nothing here uses inline assembly.
#include "common.h"
#include "kernels.h"

namespace plipmi {

namespace {

constexpr int kThreads = 256;
constexpr int kRowLanes = 16;                   // lanes per token row: one DPP row
constexpr int kRows = kThreads / kRowLanes;     // token rows per workgroup
constexpr int kChunk = 16;                      // text rows staged in LDS at a time (= kRows: one lane group per staged row's norm)
constexpr int kSlots = kTokenSimMaxC / kChunk;  // scores a lane keeps

__device__ __forceinline__ float row16_max(float v) {   // common.h row16_sum with fmaxf
  v = fmaxf(v, dpp_mov<0xB1>(v));
  v = fmaxf(v, dpp_mov<0x4E>(v));
  v = fmaxf(v, dpp_mov<0x141>(v));
  v = fmaxf(v, dpp_mov<0x140>(v));
  return v;
}
__device__ __forceinline__ float dot4(float4 a, float4 b, float acc) {
  acc = fmaf(a.x, b.x, acc);
  acc = fmaf(a.y, b.y, acc);
  acc = fmaf(a.z, b.z, acc);
  return fmaf(a.w, b.w, acc);
}

template <int NV>
__global__ __launch_bounds__(kThreads) void token_scores_kernel(const float* __restrict__ E, const float* __restrict__ T,
                                                                float* __restrict__ out, int M, int P, int C, float scale, int softmax) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float4* tl = reinterpret_cast<float4*>(smem);                                  // [kChunk][P / 4]
  float* tinv = reinterpret_cast<float*>(smem) + (size_t)kChunk * P;             // [kChunk]
  const int l16 = threadIdx.x & (kRowLanes - 1), grp = threadIdx.x / kRowLanes;
  const int row = blockIdx.x * kRows + grp;
  const int nvec = P >> 2;
  // rows past M read row M - 1 (every lane stays active for the DPP sums) and store nothing
  const float4* er = reinterpret_cast<const float4*>(E + (size_t)(row < M ? row : M - 1) * P);
  float4 ev[NV];
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int idx = l16 + kRowLanes * j;
    ev[j] = idx < nvec ? er[idx] : make_float4(0.f, 0.f, 0.f, 0.f);
    ss = dot4(ev[j], ev[j], ss);
  }
  const float einv = 1.0f / sqrtf(row16_sum(ss));

  float sc[kSlots];
#pragma unroll
  for (int k = 0; k < kSlots; ++k) sc[k] = 0.f;
#pragma unroll
  for (int k = 0; k < kSlots; ++k) {
    const int c0 = k * kChunk;
    if (c0 < C) {   // the same in every lane of the workgroup
      const int n = C - c0 < kChunk ? C - c0 : kChunk;
      if (k) __syncthreads();   // the previous chunk has been read
      const float4* src = reinterpret_cast<const float4*>(T + (size_t)c0 * P);
      for (int i = threadIdx.x; i < n * nvec; i += kThreads) tl[i] = src[i];
      __syncthreads();
      {   // lane group g: 1 / |T[c0 + g]|
        float ts = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
          const int idx = l16 + kRowLanes * j;
          const float4 t = (grp < n && idx < nvec) ? tl[grp * nvec + idx] : make_float4(0.f, 0.f, 0.f, 0.f);
          ts = dot4(t, t, ts);
        }
        ts = row16_sum(ts);
        if (l16 == 0 && grp < n) tinv[grp] = 1.0f / sqrtf(ts);
      }
      __syncthreads();
      for (int cc = 0; cc < n; ++cc) {
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
          const int idx = l16 + kRowLanes * j;
          if (idx < nvec) d = dot4(ev[j], tl[cc * nvec + idx], d);
        }
        d = row16_sum(d) * tinv[cc];
        sc[k] = cc == l16 ? d : sc[k];
      }
    }
  }

  float v[kSlots];
#pragma unroll
  for (int k = 0; k < kSlots; ++k) v[k] = scale * (sc[k] * einv);
  if (softmax) {
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < kSlots; ++k) mx = l16 + kChunk * k < C ? fmaxf(mx, v[k]) : mx;
    mx = row16_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < kSlots; ++k) {
      v[k] = l16 + kChunk * k < C ? expf(v[k] - mx) : 0.f;
      sum += v[k];
    }
    sum = row16_sum(sum);
#pragma unroll
    for (int k = 0; k < kSlots; ++k) v[k] = v[k] / sum;
  }
  if (row < M) {
    float* orow = out + (size_t)row * C;
#pragma unroll
    for (int k = 0; k < kSlots; ++k)
      if (l16 + kChunk * k < C) orow[l16 + kChunk * k] = v[k];
  }
}

template <int NV>
hipError_t token_scores(const float* E, int M, int P, const float* T, int C, float scale, int softmax, float* out, hipStream_t s) {
  const size_t lds = token_scores_lds_bytes(P);
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&token_scores_kernel<NV>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(token_scores_kernel<NV>, dim3((M + kRows - 1) / kRows), dim3(kThreads), lds, s, E, T, out, M, P, C, scale, softmax);
  return hipGetLastError();
}

}  // namespace

size_t token_scores_lds_bytes(int P) { return ((size_t)kChunk * P + kChunk) * sizeof(float); }

hipError_t launch_token_scores(const float* E, int M, int P, const float* T, int C, float scale, int softmax, float* out, hipStream_t s) {
  if (M <= 0) return hipSuccess;
  if (!E || !T || !out || P < 32 || P % 32 || P > 1024 || C < 1 || C > kTokenSimMaxC) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(E) | reinterpret_cast<uintptr_t>(T)) % 16) return hipErrorInvalidValue;
  const int nv = (P / 4 + kRowLanes - 1) / kRowLanes;   // 16-byte pieces of a row per lane
  if (nv <= 1) return token_scores<1>(E, M, P, T, C, scale, softmax, out, s);
  if (nv <= 2) return token_scores<2>(E, M, P, T, C, scale, softmax, out, s);
  if (nv <= 4) return token_scores<4>(E, M, P, T, C, scale, softmax, out, s);
  if (nv <= 8) return token_scores<8>(E, M, P, T, C, scale, softmax, out, s);
  return token_scores<16>(E, M, P, T, C, scale, softmax, out, s);
}

}  // namespace plipmi
