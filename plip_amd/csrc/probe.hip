// probe.hip -- the linear-probe head (reference: reproducibility/evaluation/linear_probing/linear_classifier.py, scikit-learn's
// SGDClassifier(loss="log_loss", penalty="l2", class_weight="balanced")): one fused loss-and-gradient pass over cached
// embeddings for all K one-vs-rest problems at once, and the predict kernel.  The solver that calls it is on the host
// (heads.hip plipmi_probe_fit).  The tile and its helpers are probe_tile.h's; the walk of probe_loss_grad_kernel described below is text
// shared with the softmax pass (probe_fit_setup.inc, probe_fit_walk.inc, probe_fit_rest.inc): this file keeps the kernel's per-thread
// constants, its residual stage and its loss reduction.
//
//   f_k(w, b) = (1/N) sum_i c_ik log(1 + exp(-t_ik (x_i.w + b))) + alpha/2 |w|^2      t_ik = +1 if y_i == k else -1
//
// probe_loss_grad_kernel<CT>: persistent workgroups of four waves walk 32-row tiles of X [N, D] fp32.  A tile is fetched from HBM
// ONCE, as 16-byte loads into registers while the previous tile is being computed, and stored to LDS ([32][Dp], Dp = D rounded up
// to 64 = 64 CT floats); both products read it from there:
//   phase 1  Z[32, 16] = X_tile W^T    v_mfma_f32_16x16x4_f32 (exact fp32), A = X rows (k = d), B = W; D is split over the four
//            waves (their W fragments stay in registers for the whole kernel), the four partial Z tiles meet in LDS;
//   residual one (row, class) pair per thread and half tile: z = b + the four partials in wave order, stable
//            log1p(exp(-|z|)) + max(-t z, 0), r = c (sigmoid(z) - [y == k]) into LDS; loss and intercept-gradient sums stay in
//            the thread, in double, for the whole kernel;
//   phase 2  G[16, D] += R^T X_tile    the same instruction, A = R^T (k = row), B = X; a wave owns CT 16-column tiles of G, whose
//            accumulators live in registers for the whole kernel.
// The LDS image of X is XOR-swizzled (column ^ probe_swz(row)) so that phase 1 (16 rows x 4 consecutive columns per wave
// read) and phase 2 (4 rows x 16 consecutive columns) are both free of bank conflicts; a 16-byte store stays contiguous.
// Every workgroup writes its partial G, g_b and loss to its own slot; probe_finish_kernel sums the slots in a FIXED order in
// double (no floating-point atomics: the same inputs give the same bits), divides by N and adds the penalty's terms (the gradient
// column is probe_tile.h's finish_grad_column, the loss tail its own).
// More than 16 problems run as ceil(K / 16) groups on grid.y, each group a pass over X of its own.
//
// probe_predict_kernel<CT>: the same tile and phase 1 for every group of 16 classes; writes the decision values [N, K] (optional)
// and the first arg-max per row (one problem: z > 0), so only [N] int32 come back to the host.
//
// A label outside [0, C) matches no problem: the row counts as a negative everywhere; y never indexes anything.
#include <algorithm>

#include "probe_tile.h"      // the shared tile: ProbeTile, its swizzle, the tile dispatch

namespace plipmi {

namespace {

template <int CT>
__global__ __launch_bounds__(kThreads) void probe_loss_grad_kernel(const float* __restrict__ X, int N, int D, const int32_t* __restrict__ y,
                                                                   const float* __restrict__ WB, int K, const float* __restrict__ pos_w,
                                                                   const float* __restrict__ neg_w, int class_base,
                                                                   float* __restrict__ part_g, double* __restrict__ part_l) {
#include "probe_fit_setup.inc"
  const float bias = live ? WB[(size_t)cls * (D + 1) + D] : 0.f;
  const float pw = live ? pos_w[cls] : 0.f, nw = live ? neg_w[cls] : 0.f;
  const int target = class_base + cls;               // the label that is positive for this problem
  double loss = 0.0, gb = 0.0;

  auto row_fetch = [](int, long) {};                 // the label is all a row's residual needs
  auto row_latch = [] {};
#include "probe_fit_walk.inc"
      float res = 0.f;
      if (live && gr < N) {
        const float z = join_scores(zp, r * kGroup + rc, bias);
        const bool pos = ycur[h] == target;
        const float c = pos ? pw : nw;
        const float e = expf(-fabsf(z));
        const float sig = z >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
        const float tz = pos ? z : -z;
        loss += (double)(c * (log1pf(e) + fmaxf(-tz, 0.f)));
        res = c * (sig - (pos ? 1.f : 0.f));
        gb += (double)res;
      }
#include "probe_fit_rest.inc"
  red[rr * kGroup + rc] = loss;
  red[256 + rr * kGroup + rc] = gb;
  __syncthreads();
  if (tid < kGroup) {                                // the problem's 16 row slots in order
    double l = 0.0, b = 0.0;
    for (int i = 0; i < 16; ++i) { l += red[i * kGroup + tid]; b += red[256 + i * kGroup + tid]; }
    pg[(size_t)tid * (D + 1) + D] = (float)b;
    part_l[(size_t)blockIdx.x * KP + kbase + tid] = l;
  }
}

// grad: finish_grad_column; loss[k] = (sum over workgroups)/N + alpha/2 |w_k|^2.  grid (K, ceil((D + 1) / 64)), 256 threads.
__global__ __launch_bounds__(256) void probe_finish_kernel(const float* __restrict__ part_g, const double* __restrict__ part_l, int nwg,
                                                          int KP, const float* __restrict__ WB, int N, int D, float alpha,
                                                          float* __restrict__ grad, double* __restrict__ loss) {
  __shared__ double sh[4][64];
  const int k = blockIdx.x, c = threadIdx.x & 63, q = threadIdx.x >> 6;
  finish_grad_column(part_g, nwg, KP, WB, N, D, alpha, grad, sh, c, q);
  if (blockIdx.y == 0 && q == 1) {       // one wave: the loss of problem k
    double l = 0.0, w2 = 0.0;
    for (int w = c; w < nwg; w += 64) l += part_l[(size_t)w * KP + k];
    for (int i = c; i < D; i += 64) { const double v = WB[(size_t)k * (D + 1) + i]; w2 += v * v; }
    l = wave_sum_f64(l);
    w2 = wave_sum_f64(w2);
    if (c == 0) loss[k] = l / N + 0.5 * (double)alpha * w2;
  }
}

template <int CT>
__global__ __launch_bounds__(kThreads) void probe_predict_kernel(const float* __restrict__ X, int N, int D, const float* __restrict__ WB,
                                                                 int K, float* __restrict__ decision, int32_t* __restrict__ pred) {
  using T = ProbeTile<CT>;
  constexpr int Dp = T::Dp;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xs = lds;
  float* zp = xs + kRows * Dp;                       // [4][32][16]
  float* best = zp + 4 * kRows * kGroup;             // [32][16] running (value, index) candidates: best[r][c], arg below
  int* arg = reinterpret_cast<int*>(best + kRows * kGroup);

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int rc = tid & 15, rr = tid >> 4;
  const long ntiles = ((long)N + kRows - 1) / kRows;
  const int groups = (K + kGroup - 1) / kGroup;
  for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    T::direct(X, N, D, t * kRows, tid, xs);
    __syncthreads();
    for (int gI = 0; gI < groups; ++gI) {
      const int kbase = gI * kGroup, cls = kbase + rc;
      float wf[T::KS];
      T::load_w(wf, WB, K, D, kbase, wave, lane);
      T::scores(xs, wf, zp, wave, lane);
      __syncthreads();
      const float bias = cls < K ? WB[(size_t)cls * (D + 1) + D] : 0.f;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int r = rr + 16 * h, o = r * kGroup + rc;
        const long gr = t * kRows + r;
        const float z = join_scores(zp, o, bias);
        if (cls < K && gr < N && decision) decision[gr * K + cls] = z;
        // column rc of the row keeps the first maximum over the problems rc, rc + 16, ... (ascending: ties keep the earlier)
        if (cls < K && (gI == 0 || z > best[o])) { best[o] = z; arg[o] = cls; }
      }
      __syncthreads();
    }
    if (tid < kRows) {
      const long gr = t * kRows + tid;
      if (gr < N) {
        if (K == 1) {
          pred[gr] = best[tid * kGroup] > 0.f ? 1 : 0;
        } else {
          float bv = best[tid * kGroup];
          int bi = arg[tid * kGroup];
          const int cols = K < kGroup ? K : kGroup;
          for (int c = 1; c < cols; ++c) {
            const float v = best[tid * kGroup + c];
            const int i = arg[tid * kGroup + c];
            if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
          }
          pred[gr] = bi;
        }
      }
    }
    __syncthreads();
  }
}

int compute_units() {
  static int cus = 0;
  if (!cus) {
    int dev = 0;
    hipDeviceProp_t p;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&p, dev) == hipSuccess) cus = p.multiProcessorCount;
    if (cus <= 0) cus = 256;
  }
  return cus;
}

}  // namespace

// 64-column blocks of the LDS row, rounded up to an instantiated tile (PROBE_DISPATCH)
int probe_col_tiles(int D) {
  const int ct = (D + 63) / 64;
  return ct <= 2 ? ct : ct <= 4 ? 4 : ct <= 6 ? 6 : ct <= 8 ? 8 : ct <= 12 ? 12 : 16;
}

// workgroups along x for N rows at width D: one per tile, at most one per CU (the kernel's registers -- next tile, W slice, G
// accumulators -- allow one workgroup per CU; its own prefetch is what overlaps the loads with the arithmetic)
int probe_workgroups(int N, int D) {
  const long ntiles = ((long)N + kRows - 1) / kRows;
  return (int)std::max<long>(1, std::min<long>(ntiles, compute_units()));
}

size_t probe_scratch_bytes(int N, int D, int K, size_t* grad_off, size_t* loss_off, size_t* partl_off) {
  const size_t KP = (size_t)((K + kGroup - 1) / kGroup) * kGroup, nwg = probe_workgroups(N, D);
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  size_t off = up(nwg * KP * (D + 1) * 4);
  *partl_off = off; off += up(nwg * KP * 8);
  *grad_off = off;  off += up((size_t)K * (D + 1) * 4);
  *loss_off = off;  off += up((size_t)K * 8);
  return off;
}

hipError_t launch_probe_loss_grad(const float* X, int N, int D, const int32_t* y, const float* WB, int K, const float* pos_w,
                                  const float* neg_w, int class_base, float alpha, char* scratch, float** grad, double** loss,
                                  hipStream_t s) {
  size_t go, lo, po;
  probe_scratch_bytes(N, D, K, &go, &lo, &po);
  float* part_g = reinterpret_cast<float*>(scratch);
  double* part_l = reinterpret_cast<double*>(scratch + po);
  *grad = reinterpret_cast<float*>(scratch + go);
  *loss = reinterpret_cast<double*>(scratch + lo);
  const int groups = (K + kGroup - 1) / kGroup, nwg = probe_workgroups(N, D);
  hipError_t e = probe_dispatch(probe_col_tiles(D), [&](auto ct) -> hipError_t {
    constexpr int CT = decltype(ct)::value;
    const size_t lds = probe_lds_bytes(CT, kRows * kGroup);              // the residuals
    if (const hipError_t e = allow_lds<&probe_loss_grad_kernel<CT>>(lds); e != hipSuccess) return e;
    probe_loss_grad_kernel<CT><<<dim3(nwg, groups), kThreads, lds, s>>>(X, N, D, y, WB, K, pos_w, neg_w, class_base, part_g, part_l);
    return hipGetLastError();
  });
  if (e != hipSuccess) return e;
  probe_finish_kernel<<<dim3(K, (D + 1 + 63) / 64), 256, 0, s>>>(part_g, part_l, nwg, groups * kGroup, WB, N, D, alpha, *grad, *loss);
  return hipGetLastError();
}

hipError_t launch_probe_predict(const float* X, int N, int D, const float* WB, int K, float* decision, int32_t* pred, hipStream_t s) {
  const long ntiles = ((long)N + kRows - 1) / kRows;
  return probe_dispatch(probe_col_tiles(D), [&](auto ct) -> hipError_t {
    constexpr int CT = decltype(ct)::value;
    const size_t lds = probe_lds_bytes(CT, 2 * kRows * kGroup);          // best and arg
    if (const hipError_t e = allow_lds<&probe_predict_kernel<CT>>(lds); e != hipSuccess) return e;
    const int nwg = (int)std::max<long>(1, std::min<long>(ntiles, (long)compute_units() * 4));
    probe_predict_kernel<CT><<<nwg, kThreads, lds, s>>>(X, N, D, WB, K, decision, pred);
    return hipGetLastError();
  });
}

}  // namespace plipmi
