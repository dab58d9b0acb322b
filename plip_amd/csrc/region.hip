// region.hip -- a slide region on the device -> the tiles that hold tissue, as the uint8 [B, t, t, 3] batch plipmi_encode_image_u8 /
// plipmi_resize_crop_u8 take.  The two entries of include/plipmi.h "slide regions" and their kernels, one unit behind everything that
// existed: no other unit's code changes.
//
//   region_count_kernel    one workgroup per grid tile: how many of its t x t pixels pass the tissue rule (integer arithmetic only;
//                          integer sums are order-free, so the count does not depend on how the pixels are spread over the lanes)
//   region_compact_kernel  ONE workgroup: the flat indices of the tiles with count >= min_count, ascending, then their number
//   region_gather_kernel   tile kept[first + b] copied into dst[b], 16 destination bytes per lane (3 t % 16 == 0: no 16-byte group
//                          crosses a tile row); region_gather_bytes_kernel: any other tile size, a byte per lane
//
// A row of the region starts at any byte (an odd pitch, x0 * 3), so the wide kernels never issue an unaligned load: src_bytes<N> reads
// the one or two ALIGNED 16-byte chunks that hold the N bytes and shifts them into place.  A chunk is only read when it holds at least
// one byte of the region, and an aligned 16-byte chunk never crosses a page: no load touches a page the region does not own.
#include <hip/hip_runtime.h>

#include "handle.h"

namespace plipmi {

struct RegionGrid {   // by value to the kernels; every product of these fits 32 bits (the region is under 4 GiB, checked on the host)
  const uint8_t* region;
  uint32_t pitch;     // bytes between rows
  int y0, x0, tile, stride, cols;
};

__device__ __forceinline__ const uint8_t* region_tile(const RegionGrid& g, int idx) {
  const int i = idx / g.cols, j = idx - i * g.cols;
  return g.region + (size_t)(g.y0 + i * g.stride) * g.pitch + (size_t)(g.x0 + j * g.stride) * 3;
}

// bytes p[0 .. N) (N <= 16) as the low bytes of four little-endian dwords, from aligned 16-byte loads only (see the file comment)
template <int N>
__device__ __forceinline__ uint4 src_bytes(const uint8_t* p) {
  const unsigned off = (unsigned)(reinterpret_cast<uintptr_t>(p) & 15);
  const uint4* q = reinterpret_cast<const uint4*>(p - off);      // (pointer arithmetic: the loads stay global_load, not flat)
  const uint4 lo = q[0];
  uint4 hi = make_uint4(0, 0, 0, 0);
  if (off + N > 16) hi = q[1];
  const unsigned k = off >> 2, sh = (off & 3) * 8;
  const uint32_t e0 = k == 0 ? lo.x : k == 1 ? lo.y : k == 2 ? lo.z : lo.w;
  const uint32_t e1 = k == 0 ? lo.y : k == 1 ? lo.z : k == 2 ? lo.w : hi.x;
  const uint32_t e2 = k == 0 ? lo.z : k == 1 ? lo.w : k == 2 ? hi.x : hi.y;
  const uint32_t e3 = k == 0 ? lo.w : k == 1 ? hi.x : k == 2 ? hi.y : hi.z;
  const uint32_t e4 = k == 0 ? hi.x : k == 1 ? hi.y : k == 2 ? hi.z : hi.w;
  return make_uint4(__funnelshift_r(e0, e1, sh), __funnelshift_r(e1, e2, sh), __funnelshift_r(e2, e3, sh), __funnelshift_r(e3, e4, sh));
}

struct TissueRule { int sat_min, luma_min, luma_max; };

__device__ __forceinline__ int is_tissue(int r, int g, int b, const TissueRule& t) {
  const int mx = max(r, max(g, b)), mn = min(r, min(g, b));
  const int luma = (77 * r + 150 * g + 29 * b + 128) >> 8;
  return (255 * (mx - mn) >= t.sat_min * mx) & (luma >= t.luma_min) & (luma <= t.luma_max);
}

__global__ __launch_bounds__(256) void region_count_kernel(RegionGrid g, TissueRule rule, int* __restrict__ counts) {
  __shared__ int part[4];
  const uint8_t* base = region_tile(g, blockIdx.x);
  const int t = g.tile, groups = (t + 3) >> 2;      // a lane takes 4 pixels = 12 bytes of a row; the row's last group may be short
  const int items = t * groups;
  int n = 0;
  for (int it = threadIdx.x; it < items; it += 256) {
    const int r = it / groups, x = (it - r * groups) * 4;
    const uint8_t* p = base + (size_t)r * g.pitch + (size_t)x * 3;
    if (x + 4 <= t) {
      const uint4 w = src_bytes<12>(p);
      n += is_tissue(w.x & 255, (w.x >> 8) & 255, (w.x >> 16) & 255, rule);
      n += is_tissue(w.x >> 24, w.y & 255, (w.y >> 8) & 255, rule);
      n += is_tissue((w.y >> 16) & 255, w.y >> 24, w.z & 255, rule);
      n += is_tissue((w.z >> 8) & 255, (w.z >> 16) & 255, w.z >> 24, rule);
    } else {
      for (int k = 0; x + k < t; ++k) n += is_tissue(p[3 * k], p[3 * k + 1], p[3 * k + 2], rule);
    }
  }
  for (int d = 32; d > 0; d >>= 1) n += __shfl_down(n, d, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// thread i owns tiles [i * per, (i + 1) * per): counts them, the 256 sums are scanned, then it writes its kept indices behind those of
// the threads before it -- ascending, whatever the number of tiles
__global__ __launch_bounds__(256) void region_compact_kernel(const int* __restrict__ counts, int n, int min_count,
                                                             int* __restrict__ kept, int* __restrict__ n_kept) {
  __shared__ int part[256];
  const int tid = threadIdx.x;
  const int per = (n + 255) / 256;
  const int lo = (long long)tid * per < n ? tid * per : n, hi = n - lo < per ? n : lo + per;
  int mine = 0;
  for (int i = lo; i < hi; ++i) mine += counts[i] >= min_count;
  part[tid] = mine;
  __syncthreads();
  if (tid == 0) {
    int acc = 0;
    for (int i = 0; i < 256; ++i) { const int v = part[i]; part[i] = acc; acc += v; }
    *n_kept = acc;
  }
  __syncthreads();
  int at = part[tid];
  for (int i = lo; i < hi; ++i)
    if (counts[i] >= min_count) kept[at++] = i;
}

// an index that is no tile of the grid (a `kept` the caller filled with something else) reads tile 0 or the last one, never a wild address
__device__ __forceinline__ int region_kept_tile(const int* __restrict__ kept, int at, int n_tiles) {
  const int idx = kept[at];
  return idx < 0 ? 0 : (idx >= n_tiles ? n_tiles - 1 : idx);
}

// grid = B * chunks; a chunk = 256 lanes x 16 bytes of one tile's 3 t^2 bytes
__global__ __launch_bounds__(256) void region_gather_kernel(RegionGrid g, int n_tiles, const int* __restrict__ kept, int first,
                                                            int chunks, uint8_t* __restrict__ dst) {
  const int b = blockIdx.x / chunks, c = blockIdx.x - b * chunks;
  const uint32_t row = 3u * g.tile, bytes = row * g.tile;
  const uint32_t o = ((uint32_t)c * 256 + threadIdx.x) * 16;
  if (o >= bytes) return;
  const uint8_t* base = region_tile(g, region_kept_tile(kept, first + b, n_tiles));
  const uint32_t r = o / row, x = o - r * row;
  *reinterpret_cast<uint4*>(dst + (size_t)b * bytes + o) = src_bytes<16>(base + (size_t)r * g.pitch + x);
}

__global__ __launch_bounds__(256) void region_gather_bytes_kernel(RegionGrid g, int n_tiles, const int* __restrict__ kept, int first,
                                                                  int chunks, uint8_t* __restrict__ dst) {
  const int b = blockIdx.x / chunks, c = blockIdx.x - b * chunks;
  const uint32_t row = 3u * g.tile, bytes = row * g.tile;
  const uint8_t* base = region_tile(g, region_kept_tile(kept, first + b, n_tiles));
  for (uint32_t o = (uint32_t)c * 4096 + threadIdx.x; o < bytes && o < ((uint32_t)c + 1) * 4096; o += 256) {
    const uint32_t r = o / row, x = o - r * row;
    dst[(size_t)b * bytes + o] = base[(size_t)r * g.pitch + x];
  }
}

// What both entries check about the region and the grid on it; `rows` x `cols` tiles.  0 or a PLIPMI_ERR_INVALID with its message.
static int check_region(const char* who, plipmi_handle h, const uint8_t* region, int H, int W, long long pitch, int y0, int x0, int tile,
                        int stride, long long rows, long long cols) {
  if (!h) return fail(PLIPMI_ERR_INVALID, "%s: null handle", who);
  if (!region) return fail(PLIPMI_ERR_INVALID, "%s: null region", who);
  if (H < 1 || W < 1) return fail(PLIPMI_ERR_INVALID, "%s: a region of %d x %d pixels", who, H, W);
  if (pitch < 3ll * W) return fail(PLIPMI_ERR_INVALID, "%s: pitch_bytes %lld is below the %lld bytes of a row of %d pixels", who, pitch, 3ll * W, W);
  if (pitch >= (1ll << 32) || pitch * H >= (1ll << 32))
    return fail(PLIPMI_ERR_INVALID, "%s: a region of %d rows of %lld bytes is 4 GiB or more (pass it in bands)", who, H, pitch);
  if (tile < 1 || stride < 1 || y0 < 0 || x0 < 0)
    return fail(PLIPMI_ERR_INVALID, "%s: tile %d, stride %d, origin (%d, %d): need tile >= 1, stride >= 1, origin >= 0", who, tile, stride, y0, x0);
  if (rows < 0 || cols < 0 || rows * cols > 0x7fffffffll) return fail(PLIPMI_ERR_INVALID, "%s: a grid of %lld x %lld tiles", who, rows, cols);
  if (rows > 0 && cols > 0 && (y0 + (rows - 1) * stride + tile > H || x0 + (cols - 1) * stride + tile > W))
    return fail(PLIPMI_ERR_INVALID, "%s: %lld x %lld tiles of %d px every %d px from (%d, %d) end at (%lld, %lld), outside the %d x %d region", who,
                rows, cols, tile, stride, y0, x0, y0 + (rows - 1) * stride + tile, x0 + (cols - 1) * stride + tile, H, W);
  return PLIPMI_OK;
}

}  // namespace plipmi

using namespace plipmi;

extern "C" {

int plipmi_region_select(plipmi_handle h, const uint8_t* region, int H, int W, int64_t pitch_bytes, int y0, int x0, int tile, int stride,
                         int rows, int cols, int sat_min, int luma_min, int luma_max, int min_count, int32_t* counts, int32_t* kept,
                         int32_t* n_kept, void* stream) {
  RUN(check_region("plipmi_region_select", h, region, H, W, pitch_bytes, y0, x0, tile, stride, rows, cols));
  if (sat_min < 0 || sat_min > 255 || luma_min < 0 || luma_min > 255 || luma_max < 0 || luma_max > 255)
    return fail(PLIPMI_ERR_INVALID, "plipmi_region_select: sat_min %d, luma_min %d, luma_max %d: each is 0 .. 255", sat_min, luma_min, luma_max);
  if (min_count < 0) return fail(PLIPMI_ERR_INVALID, "plipmi_region_select: min_count %d is negative", min_count);
  if (tile > 32768) return fail(PLIPMI_ERR_INVALID, "plipmi_region_select: tile %d: at most 32768 (the count is an int32)", tile);
  if (!n_kept) return fail(PLIPMI_ERR_INVALID, "plipmi_region_select: null n_kept");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int n = rows * cols;
  if (n == 0) {
    HIP_TRY(hipMemsetAsync(n_kept, 0, sizeof(int32_t), s));
    return PLIPMI_OK;
  }
  if (!counts || !kept) return fail(PLIPMI_ERR_INVALID, "plipmi_region_select: null counts/kept");
  const RegionGrid g{region, (uint32_t)pitch_bytes, y0, x0, tile, stride, cols};
  const TissueRule rule{sat_min, luma_min, luma_max};
  {
    Scope sc(h, s, "region_count", 0, (double)n * tile * tile * 3);
    hipLaunchKernelGGL(region_count_kernel, dim3(n), dim3(256), 0, s, g, rule, counts);
    HIP_TRY(hipGetLastError());
  }
  Scope sc(h, s, "region_compact", 0, (double)n * 12);
  hipLaunchKernelGGL(region_compact_kernel, dim3(1), dim3(256), 0, s, (const int*)counts, n, min_count, kept, n_kept);
  HIP_TRY(hipGetLastError());
  return PLIPMI_OK;
}

int plipmi_region_gather(plipmi_handle h, const uint8_t* region, int H, int W, int64_t pitch_bytes, int y0, int x0, int tile, int stride,
                         int cols, const int32_t* kept, int first, int B, uint8_t* dst, void* stream) {
  // the rows of the grid are the ones that fit: `kept` may name any tile of those rows x cols
  const long long rows = (tile >= 1 && stride >= 1 && y0 >= 0 && (long long)H - y0 - tile >= 0) ? ((long long)H - y0 - tile) / stride + 1 : 0;
  RUN(check_region("plipmi_region_gather", h, region, H, W, pitch_bytes, y0, x0, tile, stride, rows, cols));
  if (B < 0 || first < 0) return fail(PLIPMI_ERR_INVALID, "plipmi_region_gather: first %d, B %d", first, B);
  if (B == 0) return PLIPMI_OK;
  if (rows * cols == 0) return fail(PLIPMI_ERR_INVALID, "plipmi_region_gather: %d tiles of an empty grid (%lld x %d)", B, rows, cols);
  if ((long long)first + B > rows * cols)
    return fail(PLIPMI_ERR_INVALID, "plipmi_region_gather: kept[%d .. %lld) of a grid of %lld tiles", first, (long long)first + B, rows * cols);
  if (tile > 16384) return fail(PLIPMI_ERR_INVALID, "plipmi_region_gather: tile %d: at most 16384 (a tile is under 4 GiB)", tile);
  if (!kept || !dst) return fail(PLIPMI_ERR_INVALID, "plipmi_region_gather: null kept/dst");
  const size_t bytes = (size_t)3 * tile * tile;
  const size_t chunks = (bytes + 4095) / 4096;
  if (chunks * (size_t)B > 0x7fffffffull) return fail(PLIPMI_ERR_INVALID, "plipmi_region_gather: %d tiles of %d px in one call", B, tile);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const RegionGrid g{region, (uint32_t)pitch_bytes, y0, x0, tile, stride, cols};
  const bool wide = (3 * tile) % 16 == 0 && reinterpret_cast<uintptr_t>(dst) % 16 == 0;
  Scope sc(h, s, wide ? "region_gather" : "region_gather_bytes", 0, 2.0 * (double)B * (double)bytes);
  if (wide)
    hipLaunchKernelGGL(region_gather_kernel, dim3((unsigned)(chunks * B)), dim3(256), 0, s, g, (int)(rows * cols), kept, first, (int)chunks, dst);
  else
    hipLaunchKernelGGL(region_gather_bytes_kernel, dim3((unsigned)(chunks * B)), dim3(256), 0, s, g, (int)(rows * cols), kept, first,
                       (int)chunks, dst);
  HIP_TRY(hipGetLastError());
  return PLIPMI_OK;
}

}  // extern "C"
