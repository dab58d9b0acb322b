// stain.hip -- Macenko stain normalisation on the device: plipmi_stain_workspace / plipmi_stain_fit / plipmi_stain_apply of
// include/plipmi.h "stain normalisation", plipmi_stain_percentile of include/plipmi_test.h, and their kernels.  One unit behind
// everything that existed (build.py STAIN_SOURCES): no other unit calls into it and no other unit's code changes.
//
// The definition is plip_amd/preprocess.py stain_fit_reference / stain_apply_reference; this file is its restatement.  All floating
// point here is fp64 with NO contraction (every product and sum rounds once, in the order the numpy text writes them), except the
// keys, which are float32 on purpose: the oracle rounds the same values to float32 and orders those.
//
//   moments_kernel     tissue count, sum OD, sum OD (x) OD over a chunk of one image's sampled pixels -> one fp64 partial row per
//                      workgroup.  A lane adds its pixels in index order, the workgroup adds its lanes in a fixed tree: the partial
//                      does not depend on scheduling, and basis_kernel adds the partials in index order.  No floating-point atomics.
//   basis_kernel       one workgroup per fit: partials -> covariance -> cyclic Jacobi (one lane) -> e1, e2 under the sign rule
//   keys_kernel<MODE>  one float32 key per sampled pixel: 0 = the angle atan2(t1, t0) of a tissue pixel (NaN marks the others),
//                      1 / 2 = the concentration C0 / C1 of every pixel
//   hist_kernel<PASS>  radix select, 11 + 11 + 10 bits of the order-preserving uint32 image of a key: counts of the keys of one segment
//                      that carry the prefix of one rank, privatised in LDS, merged with INTEGER atomics (order-independent)
//   scan_kernel<PASS>  one workgroup per (segment, rank): the bin that holds the rank, the rank inside it; PASS 0 derives the ranks from the
//                      device-side count of present keys
//   finish_kernel      one lane per (segment, percentile): numpy's linear interpolation between the two selected keys, in fp64
//   matrix_kernel      one lane per fit: angles -> HE, det, P (steps 6 and 8 of the definition); maxima_kernel: the maxima and the flag
//   apply_kernel       C = P . lut[rgb], rescale, Io exp(-HE_t C2), min 255, truncate; PX = 4 stores dwords, WIDE loads dwords
//
// Sizes: an image is below 2 GiB (checked on the host), so offsets inside one fit an int; sample counts are size_t on the host and are
// refused above 2^31 - 8193 per call (a chunk's last lane index still fits), so every sample index fits an int too.
#include <hip/hip_runtime.h>

#include <math.h>

#include "handle.h"

namespace plipmi {

constexpr int kStainMaxQ = 8;                 // percentiles per call of the select
constexpr int kStainMaxR = 2 * kStainMaxQ;    // ranks: a[l] and a[min(l + 1, m - 1)] of each
constexpr int kBins0 = 2048, kBins2 = 1024;   // 11 + 11 + 10 bits
constexpr int kKeysPerBlock = 4096;           // 256 lanes x 16 keys
constexpr int kMomPerBlock = 16384;           // 256 lanes x 64 sampled pixels
constexpr int kMinTissue = 16;
constexpr double kMinDet = 1e-12;

struct StainSrc {            // the strided source and its sampling, by value
  const uint8_t* src;
  long long image_stride;
  int pitch;
  int H, W, step;
  int xs, ns;                // sampled columns, sampled pixels per image
  int chunks;                // workgroups per image
};

// where everything lives in the caller's workspace (offsets in bytes, every one a multiple of 256)
struct StainLayout {
  size_t keys, partials, basis, pct, maxc, sel;   // float [B ns]; double [B chunks 10]; double [F 8]; double [F 2]; double [F 2]; the select's
  size_t total;
};
struct SelectLayout {        // inside the select's part: hist0 u32 [S, 2048], hist1 u32 [S R, 2048], hist2 u32 [S R, 1024], state u32 [S R, 2], m i32 [S]
  size_t hist0, hist1, hist2, state, m;
  size_t total, zero_bytes;  // zero_bytes: the histograms, which lie first and are cleared before every select
};

static SelectLayout select_layout(size_t S, size_t R) {
  SelectLayout L;
  size_t off = 0;
  L.hist0 = off; off = align_up(off + S * kBins0 * 4, 256);
  L.hist1 = off; off = align_up(off + S * R * kBins0 * 4, 256);
  L.hist2 = off; off = align_up(off + S * R * kBins2 * 4, 256);
  L.zero_bytes = off;
  L.state = off; off = align_up(off + S * R * 8, 256);
  L.m = off; off = align_up(off + S * 4, 256);
  L.total = off;
  return L;
}

static int mom_chunks(size_t ns) { return (int)((ns + kMomPerBlock - 1) / kMomPerBlock); }

static StainLayout stain_layout(size_t B, size_t ns) {
  StainLayout L;
  size_t off = 0;
  L.keys = off; off = align_up(off + B * ns * 4, 256);
  L.partials = off; off = align_up(off + B * (size_t)mom_chunks(ns) * 10 * 8, 256);
  L.basis = off; off = align_up(off + B * 8 * 8, 256);
  L.pct = off; off = align_up(off + B * 2 * 8, 256);
  L.maxc = off; off = align_up(off + B * 2 * 8, 256);
  L.sel = off; off += select_layout(B, kStainMaxR).total;     // (B segments: what the per-image fit and the kernel-level entry use)
  L.total = off;
  return L;
}

__device__ __forceinline__ uint32_t key_bits(float f) {       // order-preserving: a < b as floats <=> key(a) < key(b) (and -0 < +0)
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ double key_value(uint32_t k) {     // back to the float's value as fp64, subnormals by integer arithmetic
  const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  const uint32_t mag = u & 0x7fffffffu;
  double v;
  if ((mag >> 23) == 0) v = (double)(int)mag * 0x1p-149;       // exact: the conversion does not depend on the fp32 denormal mode
  else v = (double)__uint_as_float(mag);
  return (u & 0x80000000u) ? -v : v;
}
__device__ __forceinline__ bool key_present(float f) { return f == f; }   // NaN = absent

// ---- moments ------------------------------------------------------------------------------------------------------------------------
// grid = B * chunks, 256 lanes; lane t of chunk c takes samples c * 16384 + t + 256 i, i = 0 .. 63, in that order
__global__ __launch_bounds__(256) void moments_kernel(StainSrc g, const double* __restrict__ lut, double beta, double* __restrict__ partials) {
#pragma clang fp contract(off)
  __shared__ double s_lut[256];
  __shared__ double s_red[256];
  s_lut[threadIdx.x] = lut[threadIdx.x];
  __syncthreads();
  const int b = blockIdx.x / g.chunks, c = blockIdx.x - b * g.chunks;
  const uint8_t* img = g.src + (size_t)b * (size_t)g.image_stride;
  double acc[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) acc[k] = 0.0;
  for (int i = 0; i < kMomPerBlock / 256; ++i) {
    const int s = c * kMomPerBlock + i * 256 + (int)threadIdx.x;
    if (s >= g.ns) break;
    const int sy = s / g.xs, sx = s - sy * g.xs;
    const uint8_t* p = img + (size_t)(sy * g.step) * (size_t)g.pitch + (size_t)(sx * g.step) * 3;
    const double o0 = s_lut[p[0]], o1 = s_lut[p[1]], o2 = s_lut[p[2]];
    if (o0 < beta || o1 < beta || o2 < beta) continue;
    acc[0] += 1.0;
    acc[1] += o0; acc[2] += o1; acc[3] += o2;
    acc[4] += o0 * o0; acc[5] += o0 * o1; acc[6] += o0 * o2;
    acc[7] += o1 * o1; acc[8] += o1 * o2; acc[9] += o2 * o2;
  }
  double* out = partials + ((size_t)b * g.chunks + c) * 10;
#pragma unroll
  for (int k = 0; k < 10; ++k) {           // a fixed tree over the 256 lanes, one quantity at a time
    s_red[threadIdx.x] = acc[k];
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
      if ((int)threadIdx.x < w) s_red[threadIdx.x] = s_red[threadIdx.x] + s_red[threadIdx.x + w];
      __syncthreads();
    }
    if (threadIdx.x == 0) out[k] = s_red[0];
    __syncthreads();
  }
}

// grid = F, 64 lanes; fit f sums partial rows f * rows_per_fit .. + rows_per_fit - 1 in index order.  basis row: e1 (3), e2 (3), n, ok
__global__ __launch_bounds__(64) void basis_kernel(const double* __restrict__ partials, int rows_per_fit, double* __restrict__ basis) {
#pragma clang fp contract(off)
  __shared__ double s_m[10];
  const int f = blockIdx.x;
  if (threadIdx.x < 10) {
    const double* p = partials + (size_t)f * rows_per_fit * 10 + threadIdx.x;
    double a = 0.0;
    int r = 0;
    for (; r + 8 <= rows_per_fit; r += 8) {         // eight loads in flight, added in index order
      double v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = p[(size_t)(r + j) * 10];
#pragma unroll
      for (int j = 0; j < 8; ++j) a += v[j];
    }
    for (; r < rows_per_fit; ++r) a += p[(size_t)r * 10];
    s_m[threadIdx.x] = a;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double* out = basis + (size_t)f * 8;
  const double n = s_m[0];
  out[6] = n;
  if (n < (double)kMinTissue) {
    for (int k = 0; k < 6; ++k) out[k] = 0.0;
    out[7] = 0.0;
    return;
  }
  const double s1[3] = {s_m[1], s_m[2], s_m[3]};
  const double s2[3][3] = {{s_m[4], s_m[5], s_m[6]}, {s_m[5], s_m[7], s_m[8]}, {s_m[6], s_m[8], s_m[9]}};
  double A[3][3], V[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      A[i][j] = (s2[i][j] - s1[i] * s1[j] / n) / (n - 1.0);
      V[i][j] = i == j ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < 16; ++sweep) {
    if (A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2] == 0.0) break;
    for (int pair = 0; pair < 3; ++pair) {
      const int p = pair == 2 ? 1 : 0, q = pair == 0 ? 1 : 2;
      const double apq = A[p][q];
      if (apq == 0.0) continue;
      const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
      double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
      if (theta < 0.0) t = -t;
      const double c = 1.0 / sqrt(t * t + 1.0);
      const double s = t * c;
      const int r = 3 - p - q;
      A[p][p] = A[p][p] - t * apq;
      A[q][q] = A[q][q] + t * apq;
      A[p][q] = A[q][p] = 0.0;
      const double arp = A[r][p], arq = A[r][q];
      A[r][p] = A[p][r] = c * arp - s * arq;
      A[r][q] = A[q][r] = s * arp + c * arq;
      for (int k = 0; k < 3; ++k) {
        const double vkp = V[k][p], vkq = V[k][q];
        V[k][p] = c * vkp - s * vkq;
        V[k][q] = s * vkp + c * vkq;
      }
    }
  }
  const double w[3] = {A[0][0], A[1][1], A[2][2]};
  int i1 = 0;
  if (w[1] > w[i1]) i1 = 1;
  if (w[2] > w[i1]) i1 = 2;                      // the first arg-max
  const int ra = i1 == 0 ? 1 : 0, rb = i1 == 2 ? 1 : 2;
  const int i2 = w[ra] >= w[rb] ? ra : rb;
  const int cols[2] = {i1, i2};
  bool finite = true;
  for (int j = 0; j < 2; ++j) {
    double e0 = V[0][cols[j]], e1 = V[1][cols[j]], e2 = V[2][cols[j]];
    if ((e0 + e1) + e2 < 0.0) { e0 = -e0; e1 = -e1; e2 = -e2; }
    out[3 * j] = e0; out[3 * j + 1] = e1; out[3 * j + 2] = e2;
    finite = finite && fabs(e0) <= 2.0 && fabs(e1) <= 2.0 && fabs(e2) <= 2.0;     // (false for a NaN)
  }
  if (!finite) for (int k = 0; k < 6; ++k) out[k] = 0.0;
  out[7] = finite ? 1.0 : 0.0;
}

// ---- keys ---------------------------------------------------------------------------------------------------------------------------
// grid = B * key chunks; sample s of image b -> keys[b * ns + s].  coef: MODE 0 the basis rows [F, 8], MODE 1 / 2 the fit rows [F, 16]
template <int MODE>
__global__ __launch_bounds__(256) void keys_kernel(StainSrc g, const double* __restrict__ lut, double beta, const double* __restrict__ coef,
                                                    int pooled, float* __restrict__ keys) {
#pragma clang fp contract(off)
  __shared__ double s_lut[256];
  s_lut[threadIdx.x] = lut[threadIdx.x];
  __syncthreads();
  const int b = blockIdx.x / g.chunks, c = blockIdx.x - b * g.chunks, f = pooled ? 0 : b;
  const uint8_t* img = g.src + (size_t)b * (size_t)g.image_stride;
  double a0, a1, a2, b0 = 0.0, b1 = 0.0, b2 = 0.0;
  if (MODE == 0) {
    const double* e = coef + (size_t)f * 8;
    a0 = e[0]; a1 = e[1]; a2 = e[2]; b0 = e[3]; b1 = e[4]; b2 = e[5];
  } else {
    const double* P = coef + (size_t)f * 16 + 6 + (MODE == 2 ? 3 : 0);
    a0 = P[0]; a1 = P[1]; a2 = P[2];
  }
  for (int i = 0; i < kKeysPerBlock / 256; ++i) {
    const int s = c * kKeysPerBlock + i * 256 + (int)threadIdx.x;
    if (s >= g.ns) break;
    const int sy = s / g.xs, sx = s - sy * g.xs;
    const uint8_t* p = img + (size_t)(sy * g.step) * (size_t)g.pitch + (size_t)(sx * g.step) * 3;
    const double o0 = s_lut[p[0]], o1 = s_lut[p[1]], o2 = s_lut[p[2]];
    float key;
    if (MODE == 0) {
      if (o0 < beta || o1 < beta || o2 < beta) {
        key = __uint_as_float(0x7fc00000u);
      } else {
        const double t0 = (o0 * a0 + o1 * a1) + o2 * a2;
        const double t1 = (o0 * b0 + o1 * b1) + o2 * b2;
        key = (float)atan2(t1, t0);
      }
    } else {
      key = (float)((a0 * o0 + a1 * o1) + a2 * o2);
    }
    keys[(size_t)b * g.ns + s] = key;
  }
}

// ---- exact percentile: radix select ------------------------------------------------------------------------------------------------------
struct SelectArgs {
  const float* keys;         // [S, n]
  uint32_t *hist0, *hist1, *hist2, *state;   // state [S R, 2] = (prefix, rank left inside the prefix)
  int32_t* m;                // [S] present keys
  int n, S, Q, R;
  double frac[kStainMaxQ];   // q / 100, divided on the host (IEEE, as numpy's true_divide)
};

// grid = kc * S for PASS 0 and kc * S * R for PASS 1 / 2, kc = the chunks of 4096 keys of a segment
template <int PASS>
__global__ __launch_bounds__(256) void hist_kernel(SelectArgs a, int kc) {
  constexpr int BINS = PASS == 2 ? kBins2 : kBins0;
  __shared__ uint32_t s_h[BINS];
  for (int i = threadIdx.x; i < BINS; i += 256) s_h[i] = 0;
  __syncthreads();
  const int sr = blockIdx.x / kc, chunk = blockIdx.x - sr * kc;
  const int seg = PASS == 0 ? sr : sr / a.R;
  uint32_t prefix = 0;
  if (PASS != 0) {
    if (a.state[(size_t)sr * 2 + 1] == 0xffffffffu) return;          // an empty segment (uniform over the workgroup)
    prefix = a.state[(size_t)sr * 2];
  }
  const float* keys = a.keys + (size_t)seg * a.n;
  for (int i = 0; i < kKeysPerBlock / 256; ++i) {
    const int s = chunk * kKeysPerBlock + i * 256 + (int)threadIdx.x;
    if (s >= a.n) break;
    const float f = keys[s];
    if (!key_present(f)) continue;
    const uint32_t k = key_bits(f);
    if (PASS == 0) atomicAdd(&s_h[k >> 21], 1u);
    else if (PASS == 1) { if ((k >> 21) == (prefix >> 21)) atomicAdd(&s_h[(k >> 10) & 2047u], 1u); }
    else { if ((k >> 10) == (prefix >> 10)) atomicAdd(&s_h[k & 1023u], 1u); }
  }
  __syncthreads();
  uint32_t* h = (PASS == 0 ? a.hist0 : PASS == 1 ? a.hist1 : a.hist2) + (size_t)sr * BINS;
  for (int i = threadIdx.x; i < BINS; i += 256)
    if (s_h[i]) atomicAdd(&h[i], s_h[i]);
}

// numpy's linear percentile from the two order statistics: every operation rounds once
__device__ __forceinline__ double lerp_numpy(double va, double vb, double t) {
#pragma clang fp contract(off)
  const double d = vb - va;
  return t < 0.5 ? va + d * t : vb - d * (1.0 - t);
}

// grid = S R, 256 lanes: one workgroup per (segment, rank).  A lane sums its BINS / 256 consecutive bins, the workgroup scans the 256 sums
// (integers: exact in any order), and the one lane whose bins hold the rank walks them.  (A single lane walking all 2048 bins measured
// 150 us a launch: 2048 dependent loads.)
// state[sr] = (the key bits found so far, the rank left inside them); a rank of 0xffffffff marks a segment without keys.
template <int PASS>
__global__ __launch_bounds__(256) void scan_kernel(SelectArgs a, int32_t* __restrict__ counts) {
#pragma clang fp contract(off)
  constexpr int BINS = PASS == 2 ? kBins2 : kBins0, PER = BINS / 256;
  __shared__ uint32_t s_sum[256];
  const int sr = blockIdx.x, t = threadIdx.x;
  const int seg = sr / a.R, r = sr - seg * a.R;
  uint32_t prefix = 0, left = 0;
  if (PASS != 0) {                                  // (uniform over the workgroup: everyone leaves before the first barrier)
    prefix = a.state[(size_t)sr * 2];
    left = a.state[(size_t)sr * 2 + 1];
    if (left == 0xffffffffu) return;
  }
  const uint32_t* h = PASS == 0 ? a.hist0 + (size_t)seg * BINS : (PASS == 1 ? a.hist1 : a.hist2) + (size_t)sr * BINS;
  uint32_t c[PER], mine = 0;
#pragma unroll
  for (int i = 0; i < PER; ++i) { c[i] = h[t * PER + i]; mine += c[i]; }
  s_sum[t] = mine;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {         // inclusive scan
    const uint32_t v = t >= off ? s_sum[t - off] : 0u;
    __syncthreads();
    s_sum[t] += v;
    __syncthreads();
  }
  const uint32_t below = s_sum[t] - mine;
  if (PASS == 0) {
    const uint32_t m = s_sum[255];
    if (r == 0 && t == 0) {
      a.m[seg] = (int32_t)m;
      if (counts) counts[seg] = (int32_t)m;
    }
    if (m == 0) {
      if (t == 0) {
        a.state[(size_t)sr * 2] = 0;
        a.state[(size_t)sr * 2 + 1] = 0xffffffffu;
      }
      return;
    }
    const double rr = a.frac[r >> 1] * (double)(m - 1);
    uint32_t l = (uint32_t)floor(rr);
    if (l > m - 1) l = m - 1;
    left = (r & 1) ? (l + 1 < m ? l + 1 : m - 1) : l;
  }
  if (left < below || left - below >= mine) return;  // not in this lane's bins (exactly one lane stays: left is below the total)
  left -= below;
  int bin = t * PER + PER - 1;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    if (left < c[i]) { bin = t * PER + i; break; }
    left -= c[i];
  }
  prefix |= (uint32_t)bin << (PASS == 0 ? 21 : PASS == 1 ? 10 : 0);
  a.state[(size_t)sr * 2] = prefix;
  a.state[(size_t)sr * 2 + 1] = left;
}

// one lane per (segment, percentile): the two selected keys -> out[seg * out_stride + q]; NaN for a segment without keys
__global__ __launch_bounds__(64) void finish_kernel(SelectArgs a, double* __restrict__ out, int out_stride) {
#pragma clang fp contract(off)
  const int sq = blockIdx.x * 64 + threadIdx.x;
  if (sq >= a.S * a.Q) return;
  const int seg = sq / a.Q, q = sq - seg * a.Q;
  const size_t sr = (size_t)seg * a.R + 2 * q;
  double* o = out + (size_t)seg * out_stride + q;
  const uint32_t m = (uint32_t)a.m[seg];
  if (m == 0) { *o = __longlong_as_double(0x7ff8000000000000ll); return; }
  const double rr = a.frac[q] * (double)(m - 1);
  double lf = floor(rr);
  if (lf > (double)(m - 1)) lf = (double)(m - 1);
  *o = lerp_numpy(key_value(a.state[sr * 2]), key_value(a.state[(sr + 1) * 2]), rr - lf);
}

// ---- stain matrix, maxima, validity ------------------------------------------------------------------------------------------------------
// one lane per fit: basis row + the two angles -> HE, P, n and a provisional valid flag in the fit row (maxC still zero)
__global__ __launch_bounds__(64) void matrix_kernel(const double* __restrict__ basis, const double* __restrict__ pct, double* __restrict__ fits, int F) {
#pragma clang fp contract(off)
  const int f = blockIdx.x * 64 + threadIdx.x;
  if (f >= F) return;
  const double* e = basis + (size_t)f * 8;
  double* row = fits + (size_t)f * 16;
  for (int k = 0; k < 16; ++k) row[k] = 0.0;
  row[14] = e[6];
  const double lo = pct[(size_t)f * 2], hi = pct[(size_t)f * 2 + 1];
  if (e[7] == 0.0 || !(fabs(lo) <= 4.0) || !(fabs(hi) <= 4.0)) return;          // (a NaN angle: no tissue keys)
  const double cl = cos(lo), sl = sin(lo), ch = cos(hi), sh = sin(hi);
  double v1[3], v2[3];
  for (int k = 0; k < 3; ++k) {
    v1[k] = e[k] * cl + e[3 + k] * sl;
    v2[k] = e[k] * ch + e[3 + k] * sh;
  }
  const bool first = v1[0] > v2[0];
  double HE[3][2];
  for (int k = 0; k < 3; ++k) {
    HE[k][0] = first ? v1[k] : v2[k];
    HE[k][1] = first ? v2[k] : v1[k];
  }
  const double a = (HE[0][0] * HE[0][0] + HE[1][0] * HE[1][0]) + HE[2][0] * HE[2][0];
  const double b = (HE[0][0] * HE[0][1] + HE[1][0] * HE[1][1]) + HE[2][0] * HE[2][1];
  const double d = (HE[0][1] * HE[0][1] + HE[1][1] * HE[1][1]) + HE[2][1] * HE[2][1];
  const double det = a * d - b * b;
  if (!(det > kMinDet)) return;
  for (int k = 0; k < 3; ++k) {
    row[2 * k] = HE[k][0];
    row[2 * k + 1] = HE[k][1];
    row[6 + k] = (d * HE[k][0] - b * HE[k][1]) / det;
    row[9 + k] = (a * HE[k][1] - b * HE[k][0]) / det;
  }
  row[15] = 1.0;
}

// one lane per fit: the maxima in, or the whole row but n cleared where one of them is not > 0
__global__ __launch_bounds__(64) void maxima_kernel(const double* __restrict__ maxc, double* __restrict__ fits, int F) {
  const int f = blockIdx.x * 64 + threadIdx.x;
  if (f >= F) return;
  double* row = fits + (size_t)f * 16;
  if (row[15] == 0.0) return;
  const double m0 = maxc[(size_t)f * 2], m1 = maxc[(size_t)f * 2 + 1];
  if (m0 > 0.0 && m1 > 0.0 && m0 < 1e300 && m1 < 1e300) {
    row[12] = m0;
    row[13] = m1;
  } else {
    for (int k = 0; k < 14; ++k) row[k] = 0.0;
    row[15] = 0.0;
  }
}

// ---- apply ------------------------------------------------------------------------------------------------------------------------------
struct ApplyArgs {
  const uint8_t* src;
  const double *fits, *target, *lut;
  uint8_t* dst;
  long long image_stride;
  double Io;
  int pitch, H, W, chunks, n_fits;
};
struct ApplyCoef { double P[6], T[6], sc[2], Io; };

__device__ __forceinline__ uint32_t stain_pixel(const double* s_lut, uint32_t rgb, const ApplyCoef& k) {   // r | g << 8 | b << 16, in and out
#pragma clang fp contract(off)
  const double o0 = s_lut[rgb & 255u], o1 = s_lut[(rgb >> 8) & 255u], o2 = s_lut[(rgb >> 16) & 255u];
  const double c0 = ((k.P[0] * o0 + k.P[1] * o1) + k.P[2] * o2) * k.sc[0];
  const double c1 = ((k.P[3] * o0 + k.P[4] * o1) + k.P[5] * o2) * k.sc[1];
  uint32_t out = 0;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    double v = k.Io * exp(-(k.T[2 * ch] * c0 + k.T[2 * ch + 1] * c1));
    v = v < 255.0 ? v : 255.0;                        // (a NaN goes to 255 like an overflow; v >= 0 always)
    out |= (uint32_t)(int)v << (8 * ch);
  }
  return out;
}

// grid = B * chunks; a chunk = 256 lanes x PX pixels of one image.  PX = 4: W % 4 == 0 and a 4-byte aligned dst, 12 bytes as three
// dwords; WIDE: the source rows are 4-byte aligned too (src, pitch and image stride all multiples of 4) and are read as dwords.
template <int PX, bool WIDE>
__global__ __launch_bounds__(256) void apply_kernel(ApplyArgs g) {
#pragma clang fp contract(off)
  __shared__ double s_lut[256];
  s_lut[threadIdx.x] = g.lut[threadIdx.x];
  __syncthreads();
  const int b = blockIdx.x / g.chunks, c = blockIdx.x - b * g.chunks;
  const int groups = g.W / PX;
  const int item = c * 256 + (int)threadIdx.x;
  if (item >= g.H * groups) return;
  const int y = item / groups, x = (item - y * groups) * PX;
  const double* fit = g.fits + (size_t)(g.n_fits == 1 ? 0 : b) * 16;
  const bool valid = fit[15] != 0.0;
  ApplyCoef k;
  if (valid) {
#pragma unroll
    for (int i = 0; i < 6; ++i) { k.P[i] = fit[6 + i]; k.T[i] = g.target[i]; }
    k.sc[0] = g.target[6] / fit[12];
    k.sc[1] = g.target[7] / fit[13];
    k.Io = g.Io;
  }
  const uint8_t* in = g.src + (size_t)b * (size_t)g.image_stride + (size_t)y * (size_t)g.pitch + (size_t)x * 3;
  uint8_t* out = g.dst + (((size_t)b * g.H + y) * g.W + x) * 3;
  uint32_t px[PX];
  if (WIDE) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(in);
    const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
    px[0] = w0 & 0xffffffu;
    if (PX == 4) {
      px[1] = (w0 >> 24) | (w1 & 0xffffu) << 8;
      px[2] = (w1 >> 16) | (w2 & 0xffu) << 16;
      px[3] = w2 >> 8;
    }
  } else {
#pragma unroll
    for (int i = 0; i < PX; ++i) px[i] = (uint32_t)in[3 * i] | (uint32_t)in[3 * i + 1] << 8 | (uint32_t)in[3 * i + 2] << 16;
  }
  if (valid) {
#pragma unroll
    for (int i = 0; i < PX; ++i) px[i] = stain_pixel(s_lut, px[i], k);
  }
  if (PX == 1) {
    out[0] = (uint8_t)px[0]; out[1] = (uint8_t)(px[0] >> 8); out[2] = (uint8_t)(px[0] >> 16);
  } else {
    uint32_t* o = reinterpret_cast<uint32_t*>(out);
    o[0] = px[0] | px[PX - 3] << 24;
    o[1] = px[PX - 3] >> 8 | px[PX - 2] << 16;
    o[2] = px[PX - 2] >> 16 | px[PX - 1] << 8;
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------
// the select over S segments of n keys each, Q percentiles per segment -> out[seg * out_stride + q]; ws = the select's part of the workspace
static int run_select(plipmi_engine* h, hipStream_t s, const float* keys, int S, int n, const double* q, int Q, double* out, int out_stride,
                      int32_t* counts, char* ws, const char* name) {
  const int R = 2 * Q;
  const SelectLayout L = select_layout((size_t)S, (size_t)R);
  SelectArgs a;
  a.keys = keys;
  a.hist0 = reinterpret_cast<uint32_t*>(ws + L.hist0);
  a.hist1 = reinterpret_cast<uint32_t*>(ws + L.hist1);
  a.hist2 = reinterpret_cast<uint32_t*>(ws + L.hist2);
  a.state = reinterpret_cast<uint32_t*>(ws + L.state);
  a.m = reinterpret_cast<int32_t*>(ws + L.m);
  a.n = n; a.S = S; a.Q = Q; a.R = R;
  for (int i = 0; i < kStainMaxQ; ++i) a.frac[i] = i < Q ? q[i] / 100.0 : 0.0;
  const long long kc = ((long long)n + kKeysPerBlock - 1) / kKeysPerBlock;
  if (kc * S * R > 0x7fffffffll) return fail(PLIPMI_ERR_INVALID, "%s: %d segments of %d keys in one call", name, S, n);
  const dim3 lanes(256), few(64);
  const dim3 scan_grid((unsigned)((long long)S * R)), fin_grid((unsigned)(((long long)S * Q + 63) / 64));
  Scope sc(h, s, name, 0.0, (double)S * n * 4.0 * (1.0 + 2.0 * R));      // the keys: once for pass 0, once per rank for passes 1 and 2
  HIP_TRY(hipMemsetAsync(ws, 0, L.zero_bytes, s));
  hipLaunchKernelGGL((hist_kernel<0>), dim3((unsigned)(kc * S)), lanes, 0, s, a, (int)kc);
  hipLaunchKernelGGL((scan_kernel<0>), scan_grid, lanes, 0, s, a, counts);
  hipLaunchKernelGGL((hist_kernel<1>), dim3((unsigned)(kc * S * R)), lanes, 0, s, a, (int)kc);
  hipLaunchKernelGGL((scan_kernel<1>), scan_grid, lanes, 0, s, a, (int32_t*)nullptr);
  hipLaunchKernelGGL((hist_kernel<2>), dim3((unsigned)(kc * S * R)), lanes, 0, s, a, (int)kc);
  hipLaunchKernelGGL((scan_kernel<2>), scan_grid, lanes, 0, s, a, (int32_t*)nullptr);
  hipLaunchKernelGGL(finish_kernel, fin_grid, few, 0, s, a, out, out_stride);
  HIP_TRY(hipGetLastError());
  return PLIPMI_OK;
}

// what plipmi_stain_fit and plipmi_stain_apply both ask of a strided batch
static int check_source(const char* who, int B, int H, int W, int64_t pitch_bytes, int64_t image_stride_bytes) {
  if (B < 0) return fail(PLIPMI_ERR_INVALID, "%s: B %d is negative", who, B);
  if (H < 1 || W < 1) return fail(PLIPMI_ERR_INVALID, "%s: images of %d x %d pixels", who, H, W);
  if (pitch_bytes < 3ll * W)
    return fail(PLIPMI_ERR_INVALID, "%s: pitch_bytes %lld is below the %lld bytes of a row of %d pixels", who, (long long)pitch_bytes, 3ll * W, W);
  if (pitch_bytes > 0x7fffffffll || pitch_bytes * H > 0x7fffffffll)
    return fail(PLIPMI_ERR_INVALID, "%s: an image of %d rows of %lld bytes is 2 GiB or more", who, H, (long long)pitch_bytes);
  if (image_stride_bytes < 0) return fail(PLIPMI_ERR_INVALID, "%s: image_stride_bytes %lld is negative", who, (long long)image_stride_bytes);
  if (B > 1 && image_stride_bytes > (int64_t)(0x7fffffffffffffffll / B))
    return fail(PLIPMI_ERR_INVALID, "%s: %d images %lld bytes apart", who, B, (long long)image_stride_bytes);
  return PLIPMI_OK;
}

static bool aligned(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

}  // namespace plipmi

using namespace plipmi;

extern "C" {

size_t plipmi_stain_workspace(int B, int H, int W, int step) {
  if (B < 1 || H < 1 || W < 1 || step < 1) return 0;
  const size_t ns = (size_t)((H + step - 1) / step) * (size_t)((W + step - 1) / step);
  return stain_layout((size_t)B, ns).total;
}

int plipmi_stain_fit(plipmi_handle h, const uint8_t* src, int B, int H, int W, int64_t pitch_bytes, int64_t image_stride_bytes, int step,
                     int pooled, double Io, double alpha, double beta, const double* lut_dev, void* workspace, double* fits_out,
                     void* stream) {
  const char* who = "plipmi_stain_fit";
  if (!h) return fail(PLIPMI_ERR_INVALID, "%s: null handle", who);
  RUN(check_source(who, B, H, W, pitch_bytes, image_stride_bytes));
  if (step < 1) return fail(PLIPMI_ERR_INVALID, "%s: step %d is below 1", who, step);
  if (pooled != 0 && pooled != 1) return fail(PLIPMI_ERR_INVALID, "%s: pooled %d is neither 0 nor 1", who, pooled);
  if (!(Io > 0.0) || !(Io < 1e300)) return fail(PLIPMI_ERR_INVALID, "%s: Io %g is not positive and finite", who, Io);
  if (!(beta > 0.0) || !(beta < 1e300)) return fail(PLIPMI_ERR_INVALID, "%s: beta %g is not positive and finite", who, beta);
  if (!(alpha > 0.0 && alpha < 50.0)) return fail(PLIPMI_ERR_INVALID, "%s: alpha %g is outside (0, 50)", who, alpha);
  const long long ys = (H + step - 1) / step, xs = (W + step - 1) / step, ns = ys * xs;
  if (ns * (long long)(B > 0 ? B : 1) > 0x7fffffffll - 8192)
    return fail(PLIPMI_ERR_INVALID, "%s: %d images of %lld sampled pixels pass 2^31 - 8193 keys in one call", who, B, ns);
  if (B == 0) return PLIPMI_OK;
  if (!src) return fail(PLIPMI_ERR_INVALID, "%s: null src", who);
  if (!lut_dev) return fail(PLIPMI_ERR_INVALID, "%s: null lut_dev", who);
  if (!workspace) return fail(PLIPMI_ERR_INVALID, "%s: null workspace", who);
  if (!fits_out) return fail(PLIPMI_ERR_INVALID, "%s: null fits_out", who);
  if (!aligned(lut_dev, 8) || !aligned(fits_out, 8) || !aligned(workspace, 16))
    return fail(PLIPMI_ERR_INVALID, "%s: lut_dev and fits_out must be 8-byte aligned and workspace 16-byte aligned", who);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int F = pooled ? 1 : B;
  const StainLayout L = stain_layout((size_t)B, (size_t)ns);
  char* ws = static_cast<char*>(workspace);
  float* keys = reinterpret_cast<float*>(ws + L.keys);
  double* partials = reinterpret_cast<double*>(ws + L.partials);
  double* basis = reinterpret_cast<double*>(ws + L.basis);
  double* pct = reinterpret_cast<double*>(ws + L.pct);
  double* maxc = reinterpret_cast<double*>(ws + L.maxc);
  StainSrc g{src, (long long)image_stride_bytes, (int)pitch_bytes, H, W, step, (int)xs, (int)ns, mom_chunks((size_t)ns)};
  const long long kc = (ns + kKeysPerBlock - 1) / kKeysPerBlock;
  const dim3 lanes(256), few(64), fit_grid((unsigned)((F + 63) / 64)), key_grid((unsigned)(kc * B));
  const double px = (double)B * (double)ns;
  {
    Scope sc(h, s, "stain_moments", px * 18.0, px * 3.0);
    hipLaunchKernelGGL(moments_kernel, dim3((unsigned)((long long)g.chunks * B)), lanes, 0, s, g, lut_dev, beta, partials);
  }
  {
    Scope sc(h, s, "stain_basis", 0.0, (double)B * g.chunks * 80.0);
    hipLaunchKernelGGL(basis_kernel, dim3((unsigned)F), few, 0, s, (const double*)partials, pooled ? B * g.chunks : g.chunks, basis);
  }
  {
    Scope sc(h, s, "stain_keys_angle", px * 12.0, px * 7.0);
    g.chunks = (int)kc;
    hipLaunchKernelGGL((keys_kernel<0>), key_grid, lanes, 0, s, g, lut_dev, beta, (const double*)basis, pooled, keys);
  }
  HIP_TRY(hipGetLastError());
  const int seg_n = (int)(pooled ? ns * B : ns);
  const double q_angle[2] = {alpha, 100.0 - alpha}, q_max[1] = {99.0};
  RUN(run_select(h, s, keys, F, seg_n, q_angle, 2, pct, 2, nullptr, ws + L.sel, "stain_select_angle"));
  hipLaunchKernelGGL(matrix_kernel, fit_grid, few, 0, s, (const double*)basis, (const double*)pct, fits_out, F);
  for (int j = 0; j < 2; ++j) {
    {
      Scope sc(h, s, "stain_keys_conc", px * 6.0, px * 7.0);
      if (j == 0) hipLaunchKernelGGL((keys_kernel<1>), key_grid, lanes, 0, s, g, lut_dev, beta, (const double*)fits_out, pooled, keys);
      else hipLaunchKernelGGL((keys_kernel<2>), key_grid, lanes, 0, s, g, lut_dev, beta, (const double*)fits_out, pooled, keys);
    }
    HIP_TRY(hipGetLastError());
    RUN(run_select(h, s, keys, F, seg_n, q_max, 1, maxc + j, 2, nullptr, ws + L.sel, "stain_select_conc"));
  }
  hipLaunchKernelGGL(maxima_kernel, fit_grid, few, 0, s, (const double*)maxc, fits_out, F);
  HIP_TRY(hipGetLastError());
  return PLIPMI_OK;
}

int plipmi_stain_apply(plipmi_handle h, const uint8_t* src, int B, int H, int W, int64_t pitch_bytes, int64_t image_stride_bytes,
                       const double* fits, int n_fits, const double* target_dev, double Io, const double* lut_dev, uint8_t* dst,
                       void* stream) {
  const char* who = "plipmi_stain_apply";
  if (!h) return fail(PLIPMI_ERR_INVALID, "%s: null handle", who);
  RUN(check_source(who, B, H, W, pitch_bytes, image_stride_bytes));
  if (!(Io > 0.0) || !(Io < 1e300)) return fail(PLIPMI_ERR_INVALID, "%s: Io %g is not positive and finite", who, Io);
  if (B == 0) return PLIPMI_OK;
  if (n_fits != 1 && n_fits != B) return fail(PLIPMI_ERR_INVALID, "%s: n_fits %d is neither 1 nor B = %d", who, n_fits, B);
  if (!src) return fail(PLIPMI_ERR_INVALID, "%s: null src", who);
  if (!fits) return fail(PLIPMI_ERR_INVALID, "%s: null fits", who);
  if (!target_dev) return fail(PLIPMI_ERR_INVALID, "%s: null target_dev", who);
  if (!lut_dev) return fail(PLIPMI_ERR_INVALID, "%s: null lut_dev", who);
  if (!dst) return fail(PLIPMI_ERR_INVALID, "%s: null dst", who);
  if (!aligned(fits, 8) || !aligned(target_dev, 8) || !aligned(lut_dev, 8))
    return fail(PLIPMI_ERR_INVALID, "%s: fits, target_dev and lut_dev must be 8-byte aligned", who);
  const long long out_px = (long long)H * W;      // (3 H W <= H pitch: below 2 GiB)
  const bool wide_st = W % 4 == 0 && aligned(dst, 4);
  const bool wide_ld = wide_st && aligned(src, 4) && pitch_bytes % 4 == 0 && image_stride_bytes % 4 == 0;
  const long long items = wide_st ? out_px / 4 : out_px;
  const long long chunks = (items + 255) / 256;
  if (chunks * B > 0x7fffffffll) return fail(PLIPMI_ERR_INVALID, "%s: %d images of %d x %d pixels in one call", who, B, H, W);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const ApplyArgs g{src, fits, target_dev, lut_dev, dst, (long long)image_stride_bytes, Io, (int)pitch_bytes, H, W, (int)chunks, n_fits};
  const dim3 grid((unsigned)(chunks * B)), block(256);
  // bytes: three read and three written per pixel; flops: the fp64 operations outside the three exponentials
  Scope sc(h, s, wide_ld ? "stain_apply" : (wide_st ? "stain_apply_bytes_in" : "stain_apply_px"), (double)B * out_px * 30.0, (double)B * out_px * 6.0);
  if (wide_ld) hipLaunchKernelGGL((apply_kernel<4, true>), grid, block, 0, s, g);
  else if (wide_st) hipLaunchKernelGGL((apply_kernel<4, false>), grid, block, 0, s, g);
  else hipLaunchKernelGGL((apply_kernel<1, false>), grid, block, 0, s, g);
  HIP_TRY(hipGetLastError());
  return PLIPMI_OK;
}

int plipmi_stain_percentile(plipmi_handle h, const float* keys, int S, int n, const double* q_host, int Q, double* out, int32_t* counts,
                            void* workspace, void* stream) {
  const char* who = "plipmi_stain_percentile";
  if (!h) return fail(PLIPMI_ERR_INVALID, "%s: null handle", who);
  if (S < 0) return fail(PLIPMI_ERR_INVALID, "%s: S %d is negative", who, S);
  if (n < 1) return fail(PLIPMI_ERR_INVALID, "%s: segments of %d keys", who, n);
  if (Q < 1 || Q > kStainMaxQ) return fail(PLIPMI_ERR_INVALID, "%s: Q %d is outside 1 .. %d", who, Q, kStainMaxQ);
  if (!q_host) return fail(PLIPMI_ERR_INVALID, "%s: null q_host", who);
  for (int i = 0; i < Q; ++i)
    if (!(q_host[i] >= 0.0 && q_host[i] <= 100.0)) return fail(PLIPMI_ERR_INVALID, "%s: q[%d] = %g is outside [0, 100]", who, i, q_host[i]);
  if ((long long)S * n > 0x7fffffffll - 8192) return fail(PLIPMI_ERR_INVALID, "%s: %d segments of %d keys pass 2^31 - 8193", who, S, n);
  if (S == 0) return PLIPMI_OK;
  if (!keys || !out || !workspace) return fail(PLIPMI_ERR_INVALID, "%s: null keys, out or workspace", who);
  if (!aligned(keys, 4) || !aligned(out, 8) || !aligned(counts, 4) || !aligned(workspace, 16))
    return fail(PLIPMI_ERR_INVALID, "%s: keys / counts must be 4-byte, out 8-byte and workspace 16-byte aligned", who);
  const StainLayout L = stain_layout((size_t)S, (size_t)n);       // the workspace of plipmi_stain_workspace(S, 1, n, 1)
  return run_select(h, reinterpret_cast<hipStream_t>(stream), keys, S, n, q_host, Q, out, Q, counts, static_cast<char*>(workspace) + L.sel,
                    "stain_select");
}

}  // extern "C"
