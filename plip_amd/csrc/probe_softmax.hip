// probe_softmax.hip -- the multinomial (softmax) linear probe: one loss-and-gradient evaluation of
//
//   f(W, b) = (1/N) sum_i cw[y_i] (logsumexp_k(x_i.w_k + b_k) - (x_i.w_{y_i} + b_{y_i})) + alpha/2 |W|_F^2
//
// at WB [C, D + 1] over cached embeddings X [N, D] fp32 -- scikit-learn's LogisticRegression(C = 1 / (alpha N)) objective, the
// cross-entropy of a linear head on a frozen tower.  The solver that calls it is on the host (heads.hip plipmi_softmax_fit).
// Unlike the one-vs-rest pass of probe.hip the C problems are coupled: a row's residual needs the log-sum-exp over ALL its classes.
//
// The tile is probe.hip's (probe_tile.h): 32 rows of X in swizzled LDS, phase 1 Z = X_tile W^T and phase 2 G += R^T X_tile with
// v_mfma_f32_16x16x4_f32 (exact fp32), G and the W slice in registers for the whole kernel, one partial slot per workgroup.  So is the
// walk of softmax_loss_grad_kernel (probe_fit_setup.inc, probe_fit_walk.inc, probe_fit_rest.inc); the kernel keeps its per-thread
// constants, the rows' statistics of the unfused form (row_fetch / row_latch), its residual stage and its loss reduction.
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
// double (no floating-point atomics: the same inputs give the same bits), divides by N and adds the penalty's terms (the gradient
// column is probe_tile.h's finish_grad_column, the loss tail its own).
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
  const int K = C;                                   // the fit walk's name for the number of problems
#include "probe_fit_setup.inc"
  const float bias = live ? WB[(size_t)cls * (D + 1) + D] : 0.f;
  const float cwk = live ? (class_w ? class_w[cls] : 1.f) : 0.f;
  double loss = 0.0, gb = 0.0;

  // unfused: the rows' statistics travel with the labels
  float mnext[2] = {0.f, 0.f}, snext[2] = {1.f, 1.f}, wnext[2] = {0.f, 0.f};
  float mcur[2], scur[2], wcur[2];
  auto row_fetch = [&](int h, long gr) {
    if constexpr (!FUSED) {
      mnext[h] = gr < N ? rowm[gr] : 0.f;
      snext[h] = gr < N ? rowsum[gr] : 1.f;
      wnext[h] = gr < N ? roww[gr] : 0.f;
    }
  };
  auto row_latch = [&] {
    if constexpr (!FUSED) {
      mcur[0] = mnext[0]; mcur[1] = mnext[1]; scur[0] = snext[0]; scur[1] = snext[1]; wcur[0] = wnext[0]; wcur[1] = wnext[1];
    }
  };
#include "probe_fit_walk.inc"
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
#include "probe_fit_rest.inc"
  red[kThreads + rr * kGroup + rc] = gb;
  if constexpr (FUSED) block_sum_to(red, loss, tid, part_l + blockIdx.x); else __syncthreads();      // part_l [gridDim.x], in thread order
  if (tid < kGroup) {
    double b = 0.0;
    for (int i = 0; i < 16; ++i) b += red[kThreads + i * kGroup + tid];
    pg[(size_t)tid * (D + 1) + D] = (float)b;
  }
}

// grad: finish_grad_column.  grid (C, ceil((D + 1) / 64)), 256 threads.  Workgroup (0, 0) then forms f = (sum of the nl loss slots) / N
// + alpha/2 |W|_F^2 with all its threads.
__global__ __launch_bounds__(256) void softmax_finish_kernel(const float* __restrict__ part_g, const double* __restrict__ part_l, int nwg,
                                                            int nl, int KP, const float* __restrict__ WB, int N, int C, int D,
                                                            float alpha, float* __restrict__ grad, double* __restrict__ loss) {
  __shared__ double sh[4][64];
  const int tid = threadIdx.x, c = tid & 63, q = tid >> 6;
  finish_grad_column(part_g, nwg, KP, WB, N, D, alpha, grad, sh, c, q);
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

constexpr size_t lds_grad(int CT) { return probe_lds_bytes(CT, kRows * kGroup); }       // the residuals
constexpr size_t lds_stats(int CT) { return probe_lds_bytes(CT, kRows * kMaxC); }       // the tile's scores, every class

struct SoftmaxScratch { size_t part_l, grad, loss, rowm, rowsum, roww, total; };

SoftmaxScratch softmax_layout(int N, int D, int C) {
  const size_t KP = (size_t)((C + kGroup - 1) / kGroup) * kGroup, nwg = probe_workgroups(N, D);
  const size_t nl = C > kGroup ? (size_t)probe_stream_workgroups(N, D) : nwg;
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
  const int nl = groups > 1 ? probe_stream_workgroups(N, D) : nwg;
  const hipError_t e = probe_dispatch(probe_col_tiles(D), [&](auto ct) -> hipError_t {
    constexpr int CT = decltype(ct)::value;
    hipError_t e;
    if (groups == 1) {
      if ((e = allow_lds<&softmax_loss_grad_kernel<CT, true>>(lds_grad(CT))) != hipSuccess) return e;
      softmax_loss_grad_kernel<CT, true><<<dim3(nwg, 1), kThreads, lds_grad(CT), s>>>(X, N, D, y, WB, C, class_w, nullptr, nullptr, nullptr,
                                                                                      part_g, part_l);
      return hipGetLastError();
    }
    if ((e = allow_lds<&softmax_stats_kernel<CT>>(lds_stats(CT))) != hipSuccess) return e;
    if ((e = allow_lds<&softmax_loss_grad_kernel<CT, false>>(lds_grad(CT))) != hipSuccess) return e;
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
