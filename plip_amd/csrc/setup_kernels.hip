// setup_kernels.hip -- the kernels that run once per handle, at plipmi_create or plipmi_clone_resolution: weight packing
// (convert, transpose, scale_copy), the LayerNorm fold into the GEMM weights, and the resampled position table.
#include "dispatch.h"
#include "kernels.h"

namespace plipmi {

// ---------------------------------------------------------------------------------
// LayerNorm folded into the neighbouring GEMMs (gemm.h EPI_*_LN), the weights' side: W'[n,:] = H(pre * (W[n,:] * g - mean_k(W[n,:] * g)))
// -- gain folded in and the row centred, so that x . W'^T == (x - mean(x)) . (W * g)^T and LayerNorm's mean subtraction needs no
// epilogue term; c2[n] = pre * (sum_k W[n,k] b[k] + bias[n]); sums in fp64.  (plipmi_create)
// ---------------------------------------------------------------------------------
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
  with_half(dtype, [&](auto tag) {
    using H = decltype(tag);
    hipLaunchKernelGGL(fold_ln_kernel<H>, dim3((rows + 3) / 4), dim3(256), 0, s, W, bias, g, b, (H*)Wf, c2, rows, K, pre);
  });
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

// ----- weight packing (plipmi_create) -----
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
  with_dtype(dst_dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(convert_kernel<T>, dim3(grid), dim3(256), 0, s, src, (T*)dst, rows, cols, dst_ld, scale);
  });
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

}  // namespace plipmi
