// augment.hip -- augmented views on the device: plipmi_warp_u8 of include/plipmi.h "augmented views" and its kernel, one unit behind
// everything that existed but region.hip: no other unit's code changes.
//
//   warp_kernel<PERSP, PX>  output pixel (x, y) of image b <- the bilinear sample of source image b (or of the ONE source image) at the
//                           point an affine / perspective row maps the pixel's centre to, inside an optional window of the source that
//                           may be mirrored left-right; outside the window: the fill colour.  The arithmetic is Pillow's
//                           Image.transform(size, AFFINE | PERSPECTIVE, coeffs, BILINEAR, fillcolor=...) (libImaging/Geometry.c:
//                           affine_transform / perspective_transform, bilinear_filter8) written out in fp64 with NO contraction: every
//                           product and sum rounds once, in the order of the numpy restatement (plip_amd/preprocess.py warp_reference),
//                           and the division is IEEE -- the bytes are Pillow's, not close to them.
//                           PX = 4: a lane makes four pixels of a row and stores their 12 bytes as three dwords (out_w % 4 == 0 and a
//                           4-byte aligned destination: byte 12 i of an image of 3 out_w out_h bytes is then 4-byte aligned);
//                           PX = 1: any out_w, three byte stores per lane.
//
// The source is read with byte loads only: a row starts at any byte (an odd pitch, a window's wx * 3), and the four taps of a pixel are
// wherever the row sends them.  Coefficients and windows are read on the device (uniform over a workgroup: scalar loads); a window that
// is not inside the source and a perspective row whose denominator is not > 0 at the four corners of the output are REFUSED there:
// that image comes out all fill, and no address outside the source is formed.
#include <hip/hip_runtime.h>

#include "handle.h"

namespace plipmi {

struct WarpArgs {           // by value to the kernel
  const uint8_t* src;
  const int32_t* windows;   // [B,5] (wy, wx, wh, ww, flip) or null: the whole source, not mirrored
  const double* coeffs;     // [B,8]
  uint8_t* dst;
  long long image_stride;   // bytes between source images; 0: every output samples the one image
  int pitch;                // bytes between source rows; H * pitch fits an int (checked on the host)
  int H, W, out_h, out_w;
  int chunks;               // workgroups per image
  uint32_t fill;            // r | g << 8 | b << 16
};

struct WarpRow {            // what a lane needs of its image once the row and the window are read
  const uint8_t* base;      // the window's first byte
  double a[8];
  int wh, ww, flip;
  bool ok;
};

// one output pixel -> its three bytes, r | g << 8 | b << 16
template <bool PERSP>
__device__ __forceinline__ uint32_t warp_pixel(const WarpRow& r, int pitch, uint32_t fill, int x, int y) {
#pragma clang fp contract(off)
  const double xin = (double)x + 0.5, yin = (double)y + 0.5;
  double xs = (r.a[0] * xin + r.a[1] * yin) + r.a[2];
  double ys = (r.a[3] * xin + r.a[4] * yin) + r.a[5];
  if (PERSP) {
    const double den = (r.a[6] * xin + r.a[7] * yin) + 1.0;
    xs = xs / den;
    ys = ys / den;
  }
  if (!(r.ok && xs >= 0.0 && xs < (double)r.ww && ys >= 0.0 && ys < (double)r.wh)) return fill;      // (NaN: outside)
  const double xf = xs - 0.5, yf = ys - 0.5;
  const double fx = floor(xf), fy = floor(yf);
  const double dx = xf - fx, dy = yf - fy;
  const int x0 = (int)fx, y0 = (int)fy;               // -1 .. ww - 1, -1 .. wh - 1
  int c0 = min(max(x0, 0), r.ww - 1), c1 = min(max(x0 + 1, 0), r.ww - 1);
  if (r.flip) { c0 = r.ww - 1 - c0; c1 = r.ww - 1 - c1; }
  const int r0 = min(max(y0, 0), r.wh - 1);
  const bool second = y0 + 1 >= 0 && y0 + 1 < r.wh;   // row y0 + 1 is NOT clipped: outside the window the first row stands for it
  const uint8_t* p0 = r.base + r0 * pitch;
  const uint8_t* p1 = r.base + (second ? y0 + 1 : r0) * pitch;
  uint32_t out = 0;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const double p00 = (double)p0[3 * c0 + ch], p01 = (double)p0[3 * c1 + ch];
    const double v1 = p00 + (p01 - p00) * dx;
    double v2 = v1;
    if (second) {
      const double p10 = (double)p1[3 * c0 + ch], p11 = (double)p1[3 * c1 + ch];
      v2 = p10 + (p11 - p10) * dx;
    }
    const double v = v1 + (v2 - v1) * dy;             // in [0, 255]: a convex combination of bytes, rounded monotonically
    out |= (uint32_t)(int)v << (8 * ch);              // truncation, as the (UINT8) cast
  }
  return out;
}

// grid = B * chunks; a chunk = 256 lanes x PX pixels of one image's out_h * out_w
template <bool PERSP, int PX>
__global__ __launch_bounds__(256) void warp_kernel(WarpArgs g) {
#pragma clang fp contract(off)
  const int b = blockIdx.x / g.chunks, c = blockIdx.x - b * g.chunks;
  const int groups = g.out_w / PX;                    // (PX = 4 is only launched with out_w % 4 == 0)
  const int item = c * 256 + threadIdx.x;
  if (item >= g.out_h * groups) return;
  const int y = item / groups, x = (item - y * groups) * PX;

  WarpRow r;
#pragma unroll
  for (int k = 0; k < 8; ++k) r.a[k] = g.coeffs[(size_t)b * 8 + k];
  int wy = 0, wx = 0;
  r.wh = g.H; r.ww = g.W; r.flip = 0;
  if (g.windows) {
    const int32_t* w = g.windows + (size_t)b * 5;
    wy = w[0]; wx = w[1]; r.wh = w[2]; r.ww = w[3]; r.flip = w[4] != 0;
  }
  // refused on the device: a window that is not inside the source (64-bit sums: any int32 values) ...
  r.ok = wy >= 0 && wx >= 0 && r.wh >= 1 && r.ww >= 1 && (long long)wy + r.wh <= g.H && (long long)wx + r.ww <= g.W;
  if (PERSP) {   // ... and a denominator that is not > 0 at the output's four corners (it is linear: then it is > 0 at every pixel)
    const double ow = (double)g.out_w, oh = (double)g.out_h;      // (a NaN or infinite a6 / a7 fails: inf * 0 is NaN at (0, 0))
    r.ok = r.ok && ((r.a[6] * 0.0 + r.a[7] * 0.0) + 1.0) > 0.0 && ((r.a[6] * ow + r.a[7] * 0.0) + 1.0) > 0.0 &&
           ((r.a[6] * 0.0 + r.a[7] * oh) + 1.0) > 0.0 && ((r.a[6] * ow + r.a[7] * oh) + 1.0) > 0.0;
  }
  if (!r.ok) { wy = 0; wx = 0; r.wh = 1; r.ww = 1; }
  r.base = g.src + (size_t)b * (size_t)g.image_stride + (size_t)wy * (size_t)g.pitch + (size_t)wx * 3;

  uint8_t* out = g.dst + ((size_t)b * g.out_h * g.out_w + (size_t)y * g.out_w + x) * 3;
  if (PX == 1) {
    const uint32_t v = warp_pixel<PERSP>(r, g.pitch, g.fill, x, y);
    out[0] = (uint8_t)v; out[1] = (uint8_t)(v >> 8); out[2] = (uint8_t)(v >> 16);
  } else {
    const uint32_t v0 = warp_pixel<PERSP>(r, g.pitch, g.fill, x, y), v1 = warp_pixel<PERSP>(r, g.pitch, g.fill, x + 1, y);
    const uint32_t v2 = warp_pixel<PERSP>(r, g.pitch, g.fill, x + 2, y), v3 = warp_pixel<PERSP>(r, g.pitch, g.fill, x + 3, y);
    uint32_t* o = reinterpret_cast<uint32_t*>(out);
    o[0] = v0 | v1 << 24;
    o[1] = v1 >> 8 | v2 << 16;
    o[2] = v2 >> 16 | v3 << 8;
  }
}

}  // namespace plipmi

using namespace plipmi;

extern "C" {

int plipmi_warp_u8(plipmi_handle h, const uint8_t* src, int B, int H, int W, int64_t pitch_bytes, int64_t image_stride_bytes,
                   const int32_t* windows, const double* coeffs, int perspective, int out_h, int out_w, uint32_t fill_rgb, uint8_t* dst,
                   void* stream) {
  const char* who = "plipmi_warp_u8";
  if (!h) return fail(PLIPMI_ERR_INVALID, "%s: null handle", who);
  if (B < 0) return fail(PLIPMI_ERR_INVALID, "%s: B %d is negative", who, B);
  if (H < 1 || W < 1) return fail(PLIPMI_ERR_INVALID, "%s: a source of %d x %d pixels", who, H, W);
  if (out_h < 1 || out_w < 1) return fail(PLIPMI_ERR_INVALID, "%s: an output of %d x %d pixels", who, out_h, out_w);
  if (pitch_bytes < 3ll * W)
    return fail(PLIPMI_ERR_INVALID, "%s: pitch_bytes %lld is below the %lld bytes of a row of %d pixels", who, (long long)pitch_bytes, 3ll * W, W);
  if (pitch_bytes > 0x7fffffffll || pitch_bytes * H > 0x7fffffffll)
    return fail(PLIPMI_ERR_INVALID, "%s: a source image of %d rows of %lld bytes is 2 GiB or more", who, H, (long long)pitch_bytes);
  if (image_stride_bytes < 0) return fail(PLIPMI_ERR_INVALID, "%s: image_stride_bytes %lld is negative", who, (long long)image_stride_bytes);
  if (B > 1 && image_stride_bytes > (int64_t)(0x7fffffffffffffffll / B))
    return fail(PLIPMI_ERR_INVALID, "%s: %d source images %lld bytes apart", who, B, (long long)image_stride_bytes);
  if (perspective != 0 && perspective != 1) return fail(PLIPMI_ERR_INVALID, "%s: perspective %d is neither 0 nor 1", who, perspective);
  if (fill_rgb > 0xffffffu) return fail(PLIPMI_ERR_INVALID, "%s: fill_rgb 0x%x has bits above its three bytes", who, fill_rgb);
  const long long out_px = (long long)out_h * out_w;
  if (out_px > 0x7fffffffll / 3) return fail(PLIPMI_ERR_INVALID, "%s: an output image of %d x %d pixels is 2 GiB or more", who, out_h, out_w);
  if (B == 0) return PLIPMI_OK;
  if (!src) return fail(PLIPMI_ERR_INVALID, "%s: null src", who);
  if (!coeffs) return fail(PLIPMI_ERR_INVALID, "%s: null coeffs", who);
  if (!dst) return fail(PLIPMI_ERR_INVALID, "%s: null dst", who);
  if (reinterpret_cast<uintptr_t>(coeffs) % 8 != 0 || reinterpret_cast<uintptr_t>(windows) % 4 != 0)
    return fail(PLIPMI_ERR_INVALID, "%s: coeffs must be 8-byte aligned and windows 4-byte aligned", who);
  const bool wide = out_w % 4 == 0 && reinterpret_cast<uintptr_t>(dst) % 4 == 0;
  const long long items = wide ? out_px / 4 : out_px;
  const long long chunks = (items + 255) / 256;
  if (chunks * B > 0x7fffffffll) return fail(PLIPMI_ERR_INVALID, "%s: %d outputs of %d x %d pixels in one call", who, B, out_h, out_w);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const WarpArgs g{src, windows, coeffs, dst, (long long)image_stride_bytes, (int)pitch_bytes, H, W, out_h, out_w, (int)chunks, fill_rgb};
  const dim3 grid((unsigned)(chunks * B)), block(256);
  // bytes: the output written, and four taps of three bytes read per pixel (most of them cache hits); flops: the fp64 operations
  Scope sc(h, s, perspective ? (wide ? "warp_perspective" : "warp_perspective_px") : (wide ? "warp_affine" : "warp_affine_px"),
           (double)B * out_px * (perspective ? 46.0 : 38.0), (double)B * out_px * 15.0);
  if (perspective) {
    if (wide) hipLaunchKernelGGL((warp_kernel<true, 4>), grid, block, 0, s, g);
    else hipLaunchKernelGGL((warp_kernel<true, 1>), grid, block, 0, s, g);
  } else {
    if (wide) hipLaunchKernelGGL((warp_kernel<false, 4>), grid, block, 0, s, g);
    else hipLaunchKernelGGL((warp_kernel<false, 1>), grid, block, 0, s, g);
  }
  HIP_TRY(hipGetLastError());
  return PLIPMI_OK;
}

}  // extern "C"
