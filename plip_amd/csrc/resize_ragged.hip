// resize_ragged.hip -- Pillow-exact 8-bit bicubic resize + centre crop of a RAGGED batch: B uint8 RGB images, each with its own
// height and width, packed end to end in one buffer -> uint8 [B, n, n, 3] tiles for plipmi_encode_image_u8 (reference:
// reproducibility/embedders/transform.py:45-48, plip.py:32-35 on lists whose sizes differ).  The uniform entry
// (head_kernels.hip resize_h_kernel / resize_v_kernel) takes host-built coefficient tables, one pair per image size; here nothing per
// size is built on the host -- four launches per batch, whatever the sizes:
//
//   ragged_plan_kernel   one workgroup: per image the resize geometry (resize_ragged.h rr_geometry), the two axis descriptors and the
//                        image's place in the intermediate buffer (exclusive prefix sum of the per-image row bounds rr_tmp_rows)
//   ragged_table_kernel  one thread per (image, axis, output position of the crop window): Pillow's bounds and 22-bit coefficients
//                        in uncontracted float64 (rr_table_row) -> bounds int32 [B, 2, n, 2], coef int32 [B, 2, n, ks]
//   ragged_h_kernel      horizontal pass over the source rows the image's vertical window reads, the n crop columns only
//   ragged_v_kernel      vertical pass -> dst
//
// Both passes keep the integer arithmetic of the uniform kernels: int32 accumulation from 2^21, arithmetic shift by 22, clamp to
// 0..255, horizontal first, uint8 in between.  An axis that already has the right size needs no special case: its table is one tap
// of 2^22, and (p * 2^22 + 2^21) >> 22 == p.
//
// Two kernels with an intermediate buffer, not one kernel that keeps the filtered rows of an output band in LDS: a band of r output
// rows needs r * sy + 4 * sy + 1 filtered source rows, so at the scales this entry admits (up to 64) a band's rows do not fit the
// LDS of a CU at any useful r and neighbouring bands would filter the same rows again and again, while the intermediate of a batch
// (about n * n * 3 * max(sy, 1) bytes per image, tens of MB for 256 images) stays in the Infinity Cache between the two passes.
//
// grid = (chunks, B): blockIdx.y is the image, so a workgroup never spans two images; the chunk count comes from the largest image of
// the batch and the workgroups of a smaller one stride over less work or leave at once.  Every index that comes from a table
// is clamped to the rows the plan reserved, so a table that disagreed with the plan could give wrong pixels, never an access
// outside the buffers.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "resize_ragged.h"

namespace plipmi {

__global__ __launch_bounds__(256) void ragged_plan_kernel(const long long* __restrict__ offsets, const int* __restrict__ hw, int B,
                                                          int n, int rule, size_t src_bytes, size_t tmp_bytes,
                                                          RaggedImg* __restrict__ img, RaggedAxis* __restrict__ axes) {
  __shared__ long long part[256];
  const int tid = threadIdx.x;
  const int per = (B + 255) / 256;
  const int lo = tid * per < B ? tid * per : B, hi = lo + per < B ? lo + per : B;
  long long sum = 0;
  for (int pass = 0; pass < 2; ++pass) {
    long long run = pass ? part[tid] : 0;
    for (int b = lo; b < hi; ++b) {
      const int h = hw[2 * b], w = hw[2 * b + 1];
      const long long off = offsets[b];
      bool ok = h >= 1 && w >= 1 && off >= 0 && (unsigned long long)off <= src_bytes &&
                (unsigned long long)h * (unsigned long long)w * 3ull <= src_bytes - (unsigned long long)off;
      int nw = 1, nh = 1, left = 0, top = 0, cap = 0;
      if (ok) {
        rr_geometry(h, w, n, rule, &nw, &nh, &left, &top);
        cap = rr_tmp_rows(h, nh, n);
      }
      const long long bytes = (long long)cap * n * 3;
      if (pass) {
        if ((unsigned long long)(run + bytes) > tmp_bytes) { ok = false; cap = 0; }   // the host sized tmp with the same bound
        RaggedImg d;
        d.src = ok ? off : 0; d.tmp = run; d.H = ok ? h : 0; d.W = ok ? w : 0; d.cap = cap; d.pad = 0;
        img[b] = d;
        RaggedAxis ax, ay;
        ax.in = ok ? w : 1; ax.out = ok ? nw : 1; ax.first = left; ax.pad = 0;
        ay.in = ok ? h : 1; ay.out = ok ? nh : 1; ay.first = top; ay.pad = 0;
        axes[2 * b] = ax;
        axes[2 * b + 1] = ay;
      }
      run += bytes;
    }
    if (!pass) {
      sum = run;
      part[tid] = sum;
      __syncthreads();
      if (tid == 0) {   // exclusive scan of the 256 per-thread sums
        long long acc = 0;
        for (int i = 0; i < 256; ++i) { const long long v = part[i]; part[i] = acc; acc += v; }
      }
      __syncthreads();
    }
  }
}

// axes != nullptr: thread t computes output position t % n of axis descriptor t / n; axes == nullptr (the kernel-level test entry):
// every thread takes `one`
__global__ __launch_bounds__(256) void ragged_table_kernel(const RaggedAxis* __restrict__ axes, RaggedAxis one, int naxes, int n,
                                                           int ks, int* __restrict__ bounds, int* __restrict__ coef) {
  const size_t total = (size_t)naxes * n;
  for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
    const RaggedAxis a = axes ? axes[t / n] : one;
    const int i = (int)(t % n);
    rr_table_row(a.in, a.out, a.first + i, ks, bounds + t * 2, coef + t * (size_t)ks);
  }
}

__device__ __forceinline__ uint8_t ragged_clip8(int acc) {
  const int v = acc >> 22;
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// rows [r0, r0 + R) of the source are the ones the image's vertical window reads: the tables' first and last rows give them
// (both ends of Pillow's windows grow with the output position)
__device__ __forceinline__ void ragged_rows(const int* __restrict__ yb, int n, int cap, int H, int* r0, int* R) {
  int a = yb[0], b = yb[2 * (n - 1)] + yb[2 * (n - 1) + 1];
  a = a < 0 ? 0 : (a > H ? H : a);
  b = b > H ? H : b;
  int r = b - a;
  r = r < 0 ? 0 : r;
  *r0 = a;
  *R = r < cap ? r : cap;
}

__global__ __launch_bounds__(256) void ragged_h_kernel(const uint8_t* __restrict__ src, const RaggedImg* __restrict__ img,
                                                       const int* __restrict__ bounds, const int* __restrict__ coef, int ks, int n,
                                                       uint8_t* __restrict__ tmp) {
  const int b = blockIdx.y;
  const RaggedImg d = img[b];
  const int* xb = bounds + (size_t)(2 * b) * n * 2;
  const int* yb = xb + (size_t)n * 2;
  const int* xk = coef + (size_t)(2 * b) * n * ks;
  int r0, R;
  ragged_rows(yb, n, d.cap, d.H, &r0, &R);
  const uint8_t* base = src + d.src;
  uint8_t* out = tmp + d.tmp;
  const int total = R * n;
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
    const int x = idx % n, y = idx / n;
    int x0 = xb[2 * x], cnt = xb[2 * x + 1];
    x0 = x0 < 0 ? 0 : x0;
    cnt = x0 + cnt > d.W ? d.W - x0 : cnt;
    const int* k = xk + (size_t)x * ks;
    const uint8_t* px = base + ((size_t)(r0 + y) * d.W + x0) * 3;
    int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
    for (int i = 0; i < cnt; ++i) {
      const int w = k[i];
      a0 += px[3 * i + 0] * w; a1 += px[3 * i + 1] * w; a2 += px[3 * i + 2] * w;
    }
    uint8_t* o = out + (size_t)idx * 3;
    o[0] = ragged_clip8(a0); o[1] = ragged_clip8(a1); o[2] = ragged_clip8(a2);
  }
}

__global__ __launch_bounds__(256) void ragged_v_kernel(const uint8_t* __restrict__ tmp, const RaggedImg* __restrict__ img,
                                                       const int* __restrict__ bounds, const int* __restrict__ coef, int ks, int n,
                                                       uint8_t* __restrict__ dst) {
  const int b = blockIdx.y;
  const RaggedImg d = img[b];
  const int* yb = bounds + (size_t)(2 * b + 1) * n * 2;
  const int* yk = coef + (size_t)(2 * b + 1) * n * ks;
  int r0, R;
  ragged_rows(yb, n, d.cap, d.H, &r0, &R);
  const uint8_t* in = tmp + d.tmp;
  uint8_t* out = dst + (size_t)b * n * n * 3;
  const int row = n * 3, total = n * row;      // (x, channel) flattened: rows of tmp are n * 3 contiguous bytes
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
    const int xc = idx % row, y = idx / row;
    int y0 = yb[2 * y] - r0, cnt = yb[2 * y + 1];
    y0 = y0 < 0 ? 0 : y0;
    cnt = y0 + cnt > R ? R - y0 : cnt;
    const int* k = yk + (size_t)y * ks;
    int a = 1 << 21;
    for (int i = 0; i < cnt; ++i) a += in[(size_t)(y0 + i) * row + xc] * k[i];
    out[idx] = ragged_clip8(a);
  }
}

hipError_t launch_ragged_tables(int in, int out, int first, int count, int ks, int* bounds, int* coef, hipStream_t s) {
  if (count <= 0) return hipSuccess;
  RaggedAxis one;
  one.in = in; one.out = out; one.first = first; one.pad = 0;
  hipLaunchKernelGGL(ragged_table_kernel, dim3((count + 255) / 256), dim3(256), 0, s, (const RaggedAxis*)nullptr, one, 1, count, ks,
                     bounds, coef);
  return hipGetLastError();
}

hipError_t launch_resize_crop_ragged(const uint8_t* src, size_t src_bytes, const int64_t* offsets, const int32_t* hw, int B, int n,
                                     int rule, int ks, int max_cap, void* workspace, const RaggedLayout& L, uint8_t* dst,
                                     hipStream_t s) {
  if (B <= 0) return hipSuccess;
  char* ws = static_cast<char*>(workspace);
  RaggedImg* img = reinterpret_cast<RaggedImg*>(ws + L.img);
  RaggedAxis* axes = reinterpret_cast<RaggedAxis*>(ws + L.axes);
  int* bounds = reinterpret_cast<int*>(ws + L.bounds);
  int* coef = reinterpret_cast<int*>(ws + L.coef);
  uint8_t* tmp = reinterpret_cast<uint8_t*>(ws + L.tmp);
  hipLaunchKernelGGL(ragged_plan_kernel, dim3(1), dim3(256), 0, s, reinterpret_cast<const long long*>(offsets), hw, B, n, rule,
                     src_bytes, L.tmp_bytes, img, axes);
  const size_t rows = (size_t)B * 2 * n;
  const int gt = (int)((rows + 255) / 256 < 4096 ? (rows + 255) / 256 : 4096);
  RaggedAxis none;
  none.in = 1; none.out = 1; none.first = 0; none.pad = 0;
  hipLaunchKernelGGL(ragged_table_kernel, dim3(gt), dim3(256), 0, s, (const RaggedAxis*)axes, none, 2 * B, n, ks, bounds, coef);
  const size_t th = (size_t)max_cap * n, tv = (size_t)n * n * 3;
  const int gh = (int)((th + 255) / 256 < 256 ? (th + 255) / 256 : 256);
  const int gv = (int)((tv + 255) / 256 < 256 ? (tv + 255) / 256 : 256);
  hipLaunchKernelGGL(ragged_h_kernel, dim3(gh, B), dim3(256), 0, s, src, (const RaggedImg*)img, (const int*)bounds, (const int*)coef,
                     ks, n, tmp);
  hipLaunchKernelGGL(ragged_v_kernel, dim3(gv, B), dim3(256), 0, s, (const uint8_t*)tmp, (const RaggedImg*)img, (const int*)bounds,
                     (const int*)coef, ks, n, dst);
  return hipGetLastError();
}

}  // namespace plipmi
