// resize_ragged.h -- geometry, limits and Pillow's coefficient arithmetic of the ragged resize (resize_ragged.hip), written once
// for the host (validation and sizing in plipmi_resize_crop_u8_ragged / plipmi_resize_ragged_workspace) and for the device (the
// plan and table kernels).  Plain C++ with no HIP types: a host-only program can include it.
//
// Every float64 expression here mirrors one line of Pillow's libImaging/Resample.c (precompute_coeffs, bicubic_filter,
// normalize_coeffs_8bpc) or of plip_amd/preprocess.py (resize_crop_plan, resample_coeffs).  Pillow is built without fused
// multiply-add and hipcc contracts a * b + c by default, so each function switches contraction off: one rounding per operation,
// the same bits on both sides.  The divisions are the default correctly rounded IEEE ones.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RR_HD __host__ __device__
#else
#define RR_HD
#endif

namespace plipmi {

constexpr int kRaggedMaxRatio = 64;       // largest in / out ratio of an axis: 2 * ceil(2 * 64) + 1 = 257 taps
constexpr int kRaggedMaxBatch = 65535;    // images per call (one grid row per image)

struct RaggedImg {    // per image, written by the plan kernel
  long long src;      // byte offset of the image in the packed source
  long long tmp;      // byte offset of its rows in the intermediate buffer
  int H, W;
  int cap;            // rows of n * 3 bytes reserved in the intermediate (0: the image is skipped)
  int pad;
};
struct RaggedAxis {   // per image and axis (0 = x, 1 = y): the table kernel's input
  int in, out, first, pad;
};

// torchvision Resize(n) / HF get_resize_output_image_size: shortest edge -> n, long edge int(n * long / short); then the first
// column / row of the centre crop by rule 0 (torchvision CenterCrop: int(round(excess / 2.0)), halves to even) or 1 (HF: excess // 2)
RR_HD inline int rr_crop_offset(int extent, int n, int rule) {
  const int e = extent - n, k = e >> 1;
  if (rule == 1 || !(e & 1)) return k;
  return (k & 1) ? k + 1 : k;
}
RR_HD inline void rr_geometry(int h, int w, int n, int rule, int* nw, int* nh, int* left, int* top) {
  if (w <= h) {
    *nw = n;
    *nh = (int)((double)((long long)n * h) / (double)w);
  } else {
    *nw = (int)((double)((long long)n * w) / (double)h);
    *nh = n;
  }
  *left = rr_crop_offset(*nw, n, rule);
  *top = rr_crop_offset(*nh, n, rule);
}

// max(scale, 1) of one axis, scale = (double)(float)in / out as precompute_coeffs takes it from its float box
RR_HD inline double rr_filterscale(int in, int out) {
  const double scale = (double)(float)in / (double)out;
  return scale < 1.0 ? 1.0 : scale;
}
RR_HD inline int rr_ksize(int in, int out) { return (int)ceil(2.0 * rr_filterscale(in, out)) * 2 + 1; }

// rows of the source that the vertical window of an image can touch, from its size alone (no table): the host sizes the
// intermediate buffer with it and the plan kernel lays the images out with it
RR_HD inline int rr_tmp_rows(int H, int nh, int n) {
#pragma clang fp contract(off)
  const double f = rr_filterscale(H, nh);
  const double r = ceil((double)(n + 1) * f) + 2.0 * ceil(2.0 * f) + 2.0;
  return r < (double)H ? (int)r : H;
}

RR_HD inline double rr_bicubic(double x) {   // bicubic_filter, a = -0.5
#pragma clang fp contract(off)
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
  if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * a;
  return 0.0;
}

// One row of precompute_coeffs + normalize_coeffs_8bpc: output position xx of an axis resampled from `in` to `out` pixels.
// bnd[0] = first input index, bnd[1] = taps; k[0 .. ks) = 22-bit fixed-point weights, zero past the taps.  The weights are summed
// in index order and computed twice instead of being kept (ks doubles per thread would live in scratch memory).
RR_HD inline void rr_table_row(int in, int out, int xx, int ks, int32_t* bnd, int32_t* k) {
#pragma clang fp contract(off)
  const double scale = (double)(float)in / (double)out;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = 2.0 * fs;
  const double ss = 1.0 / fs;
  const double center = 0.0 + ((double)xx + 0.5) * scale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in) xmax = in;
  int cnt = xmax - xmin;
  if (cnt > ks) cnt = ks;      // cannot happen with ks >= rr_ksize(in, out); keeps a wrong ks inside its row
  if (cnt < 0) cnt = 0;
  double ww = 0.0;
  for (int x = 0; x < cnt; ++x) ww += rr_bicubic(((double)(x + xmin) - center + 0.5) * ss);
  for (int x = 0; x < cnt; ++x) {
    double w = rr_bicubic(((double)(x + xmin) - center + 0.5) * ss);
    if (ww != 0.0) w = w / ww;
    k[x] = w < 0.0 ? (int32_t)(-0.5 + w * 4194304.0) : (int32_t)(0.5 + w * 4194304.0);
  }
  for (int x = cnt; x < ks; ++x) k[x] = 0;
  bnd[0] = xmin;
  bnd[1] = cnt;
}

// Host-side checks of a batch (before any launch).  Returns 0, or 1 + the index of the first bad image with *why set.
// *ks_needed = the tap count of the batch's largest per-axis scale, *max_cap = the most intermediate rows one image reserves.
inline int rr_check_batch(const int64_t* offsets, const int32_t* hw, int B, int n, int rule, size_t src_bytes, int* ks_needed,
                          int* max_cap, const char** why) {
  int ks = 0, cap = 0;
  for (int b = 0; b < B; ++b) {
    const int h = hw[2 * b], w = hw[2 * b + 1];
    if (h < 1 || w < 1) { *why = "a side is smaller than 1"; return 1 + b; }
    int nw, nh, left, top;
    rr_geometry(h, w, n, rule, &nw, &nh, &left, &top);
    if ((double)w / (double)nw > (double)kRaggedMaxRatio || (double)h / (double)nh > (double)kRaggedMaxRatio) {
      *why = "an in / out ratio is above 64";
      return 1 + b;
    }
    if (offsets) {
      const unsigned long long bytes = (unsigned long long)h * (unsigned long long)w * 3ull;
      if (offsets[b] < 0 || (unsigned long long)offsets[b] > src_bytes || bytes > src_bytes - (unsigned long long)offsets[b]) {
        *why = "offset + size runs past src_bytes";
        return 1 + b;
      }
    }
    const int kx = rr_ksize(w, nw), ky = rr_ksize(h, nh), c = rr_tmp_rows(h, nh, n);
    ks = kx > ks ? kx : ks;
    ks = ky > ks ? ky : ks;
    cap = c > cap ? c : cap;
  }
  if (ks_needed) *ks_needed = ks;
  if (max_cap) *max_cap = cap;
  return 0;
}

// Workspace layout: [RaggedImg B][RaggedAxis 2B][bounds int32 B*2*n*2][coef int32 B*2*n*ks][intermediate], each 256-byte aligned.
struct RaggedLayout {
  size_t img, axes, bounds, coef, tmp, tmp_bytes, total;
};
inline size_t rr_align(size_t x) { return (x + 255) & ~(size_t)255; }
inline RaggedLayout rr_layout(const int32_t* hw, int B, int n, int ks) {
  RaggedLayout L;
  L.img = 0;
  L.axes = L.img + rr_align((size_t)B * sizeof(RaggedImg));
  L.bounds = L.axes + rr_align((size_t)B * 2 * sizeof(RaggedAxis));
  L.coef = L.bounds + rr_align((size_t)B * 2 * n * 2 * sizeof(int32_t));
  L.tmp = L.coef + rr_align((size_t)B * 2 * n * (size_t)ks * sizeof(int32_t));
  size_t rows = 0;
  for (int b = 0; b < B; ++b) {
    const int h = hw[2 * b], w = hw[2 * b + 1];
    if (h < 1 || w < 1) continue;
    int nw, nh, left, top;
    rr_geometry(h, w, n, 0, &nw, &nh, &left, &top);      // nw, nh do not depend on the crop rule
    rows += (size_t)rr_tmp_rows(h, nh, n);
  }
  L.tmp_bytes = rows * (size_t)n * 3;
  L.total = L.tmp + rr_align(L.tmp_bytes);
  return L;
}

}  // namespace plipmi
