// probe_softmax.hip -- the multinomial (softmax) linear probe: one loss-and-gradient evaluation of
//
//   f(W, b) = (1/N) sum_i cw[y_i] (logsumexp_k(x_i.w_k + b_k) - (x_i.w_{y_i} + b_{y_i})) + alpha/2 |W|_F^2
//
// at WB [C, D + 1] over cached embeddings X [N, D] fp32 -- scikit-learn's LogisticRegression(C = 1 / (alpha N)) objective, the
// cross-entropy of a linear head on a frozen tower.  The solver that calls it is on the host (heads.hip plipmi_softmax_fit).
// Unlike the one-vs-rest pass of probe.hip the C problems are coupled: a row's residual needs the log-sum-exp over ALL its classes.
//
// The tile is probe.hip's (probe_tile.h): 32 rows of X in swizzled LDS, phase 1 Z = X_tile W^T and phase 2 G += R^T X_tile with
// v_mfma_f32_16x16x4_f32 (exact fp32), G and the W slice in registers for the whole kernel, one partial slot per workgroup.
//
//   C <= 16   softmax_loss_grad_kernel<CT, true>: X is read ONCE.  The 16 classes of a row sit in 16 adjacent lanes of the residual
//             stage (rc = tid & 15), so the row's max, its sum of exp(z - max) and its weight are four __shfl_xor steps each;
//             p = exp(z - max) / sum, r = cw[y] (p - [y == k]).
//   C > 16    softmax_stats_kernel<CT> first: every group of 16 classes against the tile in LDS, the row's C scores kept in LDS,
//             then max, sum and weight per row -> rowm / rowsum / roww [N], and the loss.  Then softmax_loss_grad_kernel<CT, false>,
//             one group of 16 classes per grid.y, reads the three values of its rows.  X is read 1 + ceil(C / 16) times; no
//             workgroup ever holds more than one group's W slice and G accumulators.
//
// The row maximum is taken before any exp.  Columns past C within a group are masked (their W is never read, their exp term is 0).
// y is only ever COMPARED with a class index the thread owns, and cw is indexed by that index: a label outside [0, C) matches
// nothing and gives its row weight 0.  The loss term of a row is formed in double (max + log(sum) - z_y) by the lane that owns class
// y.  Every workgroup writes its partial G, g_b and loss to its own slot; softmax_finish_kernel sums the slots in a FIXED order in
// double (no floating-point atomics: the same inputs give the same bits), divides by N and adds the penalty's terms.
#include <algorithm>
#include <climits>
#include <cmath>

#include "probe_tile.h"

namespace plipmi {

namespace {

constexpr int kMaxGroups = 4;                     // PLIPMI_PROBE_MAX_K / kGroup
constexpr int kMaxC = kMaxGroups * kGroup;

// over the 16 lanes that hold a row's classes = one DPP row (common.h row16_sum: pure VALU, every lane of the row ends with the same
// bits); call with all 64 lanes active
__device__ __forceinline__ float group_max(float v) {
  v = fmaxf(v, dpp_mov<0xB1>(v));   // quad_perm [1,0,3,2]
  v = fmaxf(v, dpp_mov<0x4E>(v));   // quad_perm [2,3,0,1]
  v = fmaxf(v, dpp_mov<0x141>(v));  // row_half_mirror
  v = fmaxf(v, dpp_mov<0x140>(v));  // row_mirror
  return v;
}
__device__ __forceinline__ float group_sum(float v) { return row16_sum(v); }

// the four waves' partial scores of (row r, column rc) in wave order, plus the intercept
__device__ __forceinline__ float join_scores(const float* zp, int o, float bias) {
  return bias + (((zp[o] + zp[kRows * kGroup + o]) + zp[2 * kRows * kGroup + o]) + zp[3 * kRows * kGroup + o]);
}

// the workgroup's 256 per-thread doubles summed by thread 0 in thread order; `red` is LDS of 256 doubles
__device__ __forceinline__ void block_sum_to(double* red, double v, int tid, double* out) {
  red[tid] = v;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int i = 0; i < kThreads; ++i) s += red[i];
    *out = s;
  }
}

// C > 16: rowm[i] = max_k z_ik, rowsum[i] = sum_k exp(z_ik - rowm[i]), roww[i] = cw[y_i] (0: y_i outside [0, C)); part_l[workgroup] =
// its rows' sum of roww (rowm + log rowsum - z_iy).  grid.x workgroups walk the tiles.
template <int CT>
__global__ __launch_bounds__(kThreads) void softmax_stats_kernel(const float* __restrict__ X, int N, int D, const int32_t* __restrict__ y,
                                                                 const float* __restrict__ WB, int C, const float* __restrict__ class_w,
                                                                 float* __restrict__ rowm, float* __restrict__ rowsum,
                                                                 float* __restrict__ roww, double* __restrict__ part_l) {
  using T = ProbeTile<CT>;
  constexpr int Dp = T::Dp;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xs = lds;
  float* zp = xs + kRows * Dp;                       // [4][32][16] partial scores; at the end: the loss reduction
  float* za = zp + 4 * kRows * kGroup;               // [32][64] the tile's scores, every class

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int rc = tid & 15, rr = tid >> 4;
  const long ntiles = ((long)N + kRows - 1) / kRows;
  const int groups = (C + kGroup - 1) / kGroup;
  double loss = 0.0;
  for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    T::direct(X, N, D, t * kRows, tid, xs);
    __syncthreads();
    for (int gI = 0; gI < groups; ++gI) {
      const int kbase = gI * kGroup, cls = kbase + rc;
      float wf[T::KS];
      T::load_w(wf, WB, C, D, kbase, wave, lane);
      T::scores(xs, wf, zp, wave, lane);
      __syncthreads();
      if (cls < C) {
        const float bias = WB[(size_t)cls * (D + 1) + D];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int r = rr + 16 * h;
          za[r * kMaxC + cls] = join_scores(zp, r * kGroup + rc, bias);
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int r = rr + 16 * h;
      const long gr = t * kRows + r;
      const int yv = gr < N ? y[gr] : -1;
      float m = -INFINITY;
      for (int cls = rc; cls < C; cls += kGroup) m = fmaxf(m, za[r * kMaxC + cls]);
      m = group_max(m);                                // C > 16: every lane owns a live class, m is a score
      float s = 0.f, w = 0.f, zy = 0.f;
      bool mine = false;                               // this lane owns class y
      for (int cls = rc; cls < C; cls += kGroup) {
        const float z = za[r * kMaxC + cls];
        s += expf(z - m);
        if (cls == yv) { mine = true; w = class_w ? class_w[cls] : 1.f; zy = z; }
      }
      s = group_sum(s);
      if (mine && gr < N) loss += (double)w * (((double)m + log((double)s)) - (double)zy);
      w = group_sum(w);                                // one non-zero term at most: exact
      if (rc == 0 && gr < N) { rowm[gr] = m; rowsum[gr] = s; roww[gr] = w; }
    }
    __syncthreads();
  }
  block_sum_to(reinterpret_cast<double*>(zp), loss, tid, part_l + blockIdx.x);
}

// FUSED (C <= 16, grid.y == 1): the whole evaluation.  Otherwise group blockIdx.y of 16 classes, the rows' statistics from
// softmax_stats_kernel, and no loss.  part_g [gridDim.x][KP][D + 1]; part_l [gridDim.x] (FUSED only).
template <int CT, bool FUSED>
__global__ __launch_bounds__(kThreads) void softmax_loss_grad_kernel(const float* __restrict__ X, int N, int D, const int32_t* __restrict__ y,
                                                                     const float* __restrict__ WB, int C, const float* __restrict__ class_w,
                                                                     const float* __restrict__ rowm, const float* __restrict__ rowsum,
                                                                     const float* __restrict__ roww, float* __restrict__ part_g,
                                                                     double* __restrict__ part_l) {
  using T = ProbeTile<CT>;
  constexpr int Dp = T::Dp;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xs = lds;                                   // [32][Dp], swizzled
  float* zp = xs + kRows * Dp;                       // [4][32][16] partial scores; at the end: the loss / g_b reduction
  float* rs = zp + 4 * kRows * kGroup;               // [32][16] residuals

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int kbase = blockIdx.y * kGroup, KP = gridDim.y * kGroup;
  const long ntiles = ((long)N + kRows - 1) / kRows;

  float wf[T::KS];
  T::load_w(wf, WB, C, D, kbase, wave, lane);
  f32x4 g[CT];
#pragma unroll
  for (int j = 0; j < CT; ++j) g[j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // residual stage: this thread's class and its two rows of a tile
  const int rc = tid & 15, rr = tid >> 4, cls = kbase + rc;
  const bool live = cls < C;
  const float bias = live ? WB[(size_t)cls * (D + 1) + D] : 0.f;
  const float cwk = live ? (class_w ? class_w[cls] : 1.f) : 0.f;
  double loss = 0.0, gb = 0.0;

  // D <= 512: the next tile waits in registers while this one is computed; wider rows need those registers for wf and g
  constexpr bool kPrefetch = CT <= 8;
  T tile;
  long t = blockIdx.x;
  int ynext[2] = {-1, -1};
  float mnext[2] = {0.f, 0.f}, snext[2] = {1.f, 1.f}, wnext[2] = {0.f, 0.f};
  auto fetch = [&](long tl) {
    if constexpr (kPrefetch) tile.fetch(X, N, D, tl * kRows, tid);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const long gr = tl * kRows + rr + 16 * h;
      ynext[h] = gr < N ? y[gr] : -1;
      if constexpr (!FUSED) {
        mnext[h] = gr < N ? rowm[gr] : 0.f;
        snext[h] = gr < N ? rowsum[gr] : 1.f;
        wnext[h] = gr < N ? roww[gr] : 0.f;
      }
    }
  };
  if (t < ntiles) fetch(t);
  while (t < ntiles) {
    if constexpr (kPrefetch) tile.stage(xs, tid); else T::direct(X, N, D, t * kRows, tid, xs);
    const int ycur[2] = {ynext[0], ynext[1]};
    const float mcur[2] = {mnext[0], mnext[1]}, scur[2] = {snext[0], snext[1]}, wcur[2] = {wnext[0], wnext[1]};
    __syncthreads();
    const long next = t + gridDim.x;
    if (next < ntiles) fetch(next);     // in flight under this tile's arithmetic
    T::scores(xs, wf, zp, wave, lane);
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int r = rr + 16 * h;
      const long gr = t * kRows + r;
      const float z = join_scores(zp, r * kGroup + rc, bias);
      const bool pos = live && ycur[h] == cls;
      float m, s, w;
      if constexpr (FUSED) {          // every lane takes part in the shuffles; a masked column is -inf / 0
        m = group_max(live ? z : -INFINITY);
        s = group_sum(live ? expf(z - m) : 0.f);
        w = group_sum(pos ? cwk : 0.f);
      } else {
        m = mcur[h]; s = scur[h]; w = wcur[h];
      }
      float res = 0.f;
      if (live && gr < N) {
        res = w * (expf(z - m) / s - (pos ? 1.f : 0.f));
        gb += (double)res;
      }
      if constexpr (FUSED) {          // outside the branches: some lane of every wave owns a label, and the two rows' logs interleave
        const double term = ((double)m + log((double)s)) - (double)z;
        if (pos && gr < N) loss += (double)cwk * term;
      }
      rs[r * kGroup + rc] = res;
    }
    __syncthreads();
    // phase 2: G[class][d] += sum_row R[row][class] X[row][d]
    {
      const int m = lane & 15, k = lane >> 4;
#pragma unroll
      for (int q = 0; q < kRows / 4; ++q) {
        const int row = 4 * q + k;
        const float a = rs[row * kGroup + m];
        const float* xr = xs + row * Dp;
        const int sw = probe_swz(row);
#pragma unroll
        for (int j = 0; j < CT; ++j) g[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, xr[((wave * CT + j) * 16 + m) ^ sw], g[j], 0, 0, 0);
      }
    }
    __syncthreads();
    t = next;
  }

  // this workgroup's slot
  float* pg = part_g + ((size_t)blockIdx.x * KP + kbase) * (D + 1);
  {
    const int m = lane & 15, k = lane >> 4;
#pragma unroll
    for (int j = 0; j < CT; ++j) {
      const int d = (wave * CT + j) * 16 + m;
      if (d < D) {
#pragma unroll
        for (int i = 0; i < 4; ++i) pg[(size_t)(4 * k + i) * (D + 1) + d] = g[j][i];     // C/D: row (class) = 4 (lane >> 4) + i
      }
    }
  }
  double* red = reinterpret_cast<double*>(zp);        // [2][256] doubles = 4 KiB of zp's 8 KiB
  red[kThreads + rr * kGroup + rc] = gb;
  if constexpr (FUSED) block_sum_to(red, loss, tid, part_l + blockIdx.x); else __syncthreads();
  if (tid < kGroup) {
    double b = 0.0;
    for (int i = 0; i < 16; ++i) b += red[kThreads + i * kGroup + tid];
    pg[(size_t)tid * (D + 1) + D] = (float)b;
  }
}

// grad[k][d] = (sum over workgroups, in order) / N + alpha W[k][d]; the intercepts have no penalty.  grid (C, ceil((D + 1) / 64)),
// 256 threads = 64 columns x 4 slices of the workgroups.  Workgroup (0, 0) then forms f = (sum of the nl loss slots) / N +
// alpha/2 |W|_F^2 with all its threads.
__global__ __launch_bounds__(256) void softmax_finish_kernel(const float* __restrict__ part_g, const double* __restrict__ part_l, int nwg,
                                                            int nl, int KP, const float* __restrict__ WB, int N, int C, int D,
                                                            float alpha, float* __restrict__ grad, double* __restrict__ loss) {
  __shared__ double sh[4][64];
  const int k = blockIdx.x, tid = threadIdx.x, c = tid & 63, q = tid >> 6;
  const int d = blockIdx.y * 64 + c;
  double acc = 0.0;
  if (d <= D) {
    const int w0 = (int)((long)nwg * q / 4), w1 = (int)((long)nwg * (q + 1) / 4);
    for (int w = w0; w < w1; ++w) acc += (double)part_g[((size_t)w * KP + k) * (D + 1) + d];
  }
  sh[q][c] = acc;
  __syncthreads();
  if (q == 0 && d <= D) {
    const double s = ((sh[0][c] + sh[1][c]) + sh[2][c]) + sh[3][c];
    const double pen = d < D ? (double)alpha * (double)WB[(size_t)k * (D + 1) + d] : 0.0;
    grad[(size_t)k * (D + 1) + d] = (float)(s / N + pen);
  }
  if (blockIdx.x == 0 && blockIdx.y == 0) {
    __syncthreads();
    double l = 0.0, w2 = 0.0;
    for (int w = tid; w < nl; w += 256) l += part_l[w];
    for (int i = tid; i < C * D; i += 256) { const double v = WB[(size_t)(i / D) * (D + 1) + i % D]; w2 += v * v; }
    l = wave_sum_f64(l);
    w2 = wave_sum_f64(w2);
    if (c == 0) { sh[0][q] = l; sh[1][q] = w2; }
    __syncthreads();
    if (tid == 0)
      *loss = (((sh[0][0] + sh[0][1]) + sh[0][2]) + sh[0][3]) / N + 0.5 * (double)alpha * (((sh[1][0] + sh[1][1]) + sh[1][2]) + sh[1][3]);
  }
}

size_t lds_grad(int CT) { return ((size_t)kRows * 64 * CT + 4 * kRows * kGroup + kRows * kGroup) * 4; }
size_t lds_stats(int CT) { return ((size_t)kRows * 64 * CT + 4 * kRows * kGroup + kRows * kMaxC) * 4; }

// workgroups of the statistics pass: it keeps no accumulators, two per compute unit hide its loads
int stats_workgroups(int N, int D) {
  const long ntiles = ((long)N + kRows - 1) / kRows;
  return (int)std::max<long>(1, std::min<long>(ntiles, 2L * probe_workgroups(INT_MAX, D)));
}

struct SoftmaxScratch { size_t part_l, grad, loss, rowm, rowsum, roww, total; };

SoftmaxScratch softmax_layout(int N, int D, int C) {
  const size_t KP = (size_t)((C + kGroup - 1) / kGroup) * kGroup, nwg = probe_workgroups(N, D);
  const size_t nl = C > kGroup ? (size_t)stats_workgroups(N, D) : nwg;
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  SoftmaxScratch L;
  size_t off = up(nwg * KP * (D + 1) * 4);
  L.part_l = off; off += up(nl * 8);
  L.grad = off;   off += up((size_t)C * (D + 1) * 4);
  L.loss = off;   off += up(8);
  const size_t rows = C > kGroup ? up((size_t)N * 4) : 0;
  L.rowm = off;   off += rows;
  L.rowsum = off; off += rows;
  L.roww = off;   off += rows;
  L.total = off;
  return L;
}

template <typename K> hipError_t allow_lds(K kernel, size_t lds, bool* done) {
  if (*done) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e == hipSuccess) *done = true;
  return e;
}

}  // namespace

size_t softmax_scratch_bytes(int N, int D, int C) { return softmax_layout(N, D, C).total; }

hipError_t launch_softmax_loss_grad(const float* X, int N, int D, const int32_t* y, const float* WB, int C, const float* class_w,
                                    float alpha, char* scratch, float** grad, double** loss, hipStream_t s) {
  const SoftmaxScratch L = softmax_layout(N, D, C);
  float* part_g = reinterpret_cast<float*>(scratch);
  double* part_l = reinterpret_cast<double*>(scratch + L.part_l);
  float* rowm = reinterpret_cast<float*>(scratch + L.rowm);
  float* rowsum = reinterpret_cast<float*>(scratch + L.rowsum);
  float* roww = reinterpret_cast<float*>(scratch + L.roww);
  *grad = reinterpret_cast<float*>(scratch + L.grad);
  *loss = reinterpret_cast<double*>(scratch + L.loss);
  const int groups = (C + kGroup - 1) / kGroup, nwg = probe_workgroups(N, D);
  const int nl = groups > 1 ? stats_workgroups(N, D) : nwg;
  const hipError_t e = probe_dispatch(probe_col_tiles(D), [&](auto ct) -> hipError_t {
    constexpr int CT = decltype(ct)::value;
    hipError_t e;
    if (groups == 1) {
      static bool done = false;
      if ((e = allow_lds(&softmax_loss_grad_kernel<CT, true>, lds_grad(CT), &done)) != hipSuccess) return e;
      softmax_loss_grad_kernel<CT, true><<<dim3(nwg, 1), kThreads, lds_grad(CT), s>>>(X, N, D, y, WB, C, class_w, nullptr, nullptr, nullptr,
                                                                                      part_g, part_l);
      return hipGetLastError();
    }
    static bool done_s = false, done_g = false;
    if ((e = allow_lds(&softmax_stats_kernel<CT>, lds_stats(CT), &done_s)) != hipSuccess) return e;
    if ((e = allow_lds(&softmax_loss_grad_kernel<CT, false>, lds_grad(CT), &done_g)) != hipSuccess) return e;
    softmax_stats_kernel<CT><<<nl, kThreads, lds_stats(CT), s>>>(X, N, D, y, WB, C, class_w, rowm, rowsum, roww, part_l);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    softmax_loss_grad_kernel<CT, false><<<dim3(nwg, groups), kThreads, lds_grad(CT), s>>>(X, N, D, y, WB, C, class_w, rowm, rowsum, roww,
                                                                                          part_g, part_l);
    return hipGetLastError();
  });
  if (e != hipSuccess) return e;
  softmax_finish_kernel<<<dim3(C, (D + 1 + 63) / 64), 256, 0, s>>>(part_g, part_l, nwg, nl, groups * kGroup, WB, N, C, D, alpha, *grad, *loss);
  return hipGetLastError();
}

}  // namespace plipmi
