// head_kernels.hip -- the kernels that run on finished embeddings or in front of the image entry, none of them part of a tower
// forward: logits, arg-max, the two top-k forms, the Pillow-exact resize passes, and the queue probe occupy_kernel.
#include <limits.h>

#include "kernels.h"

namespace plipmi {

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

}  // namespace plipmi
