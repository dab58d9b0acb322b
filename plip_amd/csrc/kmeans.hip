// kmeans.hip -- k-means (Lloyd) on cached embeddings X [N, D] fp32: the entries of include/plipmi.h "k-means on cached embeddings", the
// update-step test entry of plipmi_test.h, and their kernels.  One unit behind every other one (no unit of build.py's SOURCES calls into
// it).  The tile, the centres' 16-byte operand form (ProbeTile load_centres / tile_scores), join_scores, the thread-order sum, the LDS
// byte count and the streaming workgroup count are probe_tile.h's; the X / N / D check is handle.h's check_embeddings.
//
// Both metrics are ONE score with a per-centre bias: s_ik = x_i . c_k + h_k (Euclidean h_k = -1/2 |c_k|^2, cosine h_k = 0), the label
// is the first arg-max over k, and the distance is recovered from the best score (|x_i|^2 - 2 s or 1 - s, clamped at 0).
//
//   assignment   kmeans_assign_kernel<CT>: probe_tile.h's 32-row tile of X in swizzled LDS (X is read ONCE), the centres stream past in
//                groups of 16 (each wave holds its column slice of the group in registers, read 16 bytes per lane; the next group's
//                slice is in flight under this group's MFMAs), products are v_mfma_f32_16x16x4_f32 (exact fp32), the four waves' partial scores are joined in wave
//                order, and every thread keeps the running best of ITS column (k mod 16) for its two rows in registers; the 16 columns
//                of a row are merged once per tile (larger score wins, equal scores: the lower k).  There is no N x K buffer.
//   update       a STABLE counting sort of the rows by label -- per-block histograms (integer LDS atomics: integer sums do not depend
//                on their order), an exclusive scan over blocks then over clusters, a ranked scatter (a row's rank among the rows of
//                its label in its 256-row batch is counted, never raced for) -- then per-cluster sums over ASCENDING rows in chunks of
//                256 members: inside a chunk, slice j of the threads adds rows j, j + S, ... in fp32, the slices are added in slice
//                order, the chunks of a cluster are added in chunk order in double and rounded once.  rep = the member with the largest
//                score, ties to the lower row (a total order: any merge order gives the same member).
//   finalise     centres from sums and counts (mean; or sum / |sum|), the shift sum_k |delta c_k|^2 in double, the empty flags.
//   seeding      plain k-means++: per step one pass that lowers mind and sums it per block in double (run sums of consecutive rows,
//                runs in order), and one workgroup that walks the block sums, the run sums and the rows in that same association to
//                the first row whose prefix exceeds u_t * total.
//
// No floating-point atomics anywhere; the one integer atomic whose value leaves a kernel is a COUNT (changed labels).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "handle.h"
#include "probe_tile.h"

namespace plipmi {

namespace {

constexpr int kChunk = 256;          // members per chunk of the per-cluster sums

// what a fit reads back per iteration
struct KmStatus {
  int32_t changed, n_empty;
  double shift, inertia;
};

__device__ __forceinline__ float km_dist(int metric, float xn, float s) {
  return metric == PLIPMI_KMEANS_EUCLIDEAN ? fmaxf(0.f, xn - 2.f * s) : fmaxf(0.f, 1.f - s);
}

// <a, b> over D columns by one wave: lane l takes the 16-byte groups l, l + 64, ..., then a butterfly.  The order is a function of D
// alone, so wave_dot(x, x) is bit for bit the row norm the same routine stored earlier.
__device__ __forceinline__ float wave_dot(const float* __restrict__ a, const float* __restrict__ b, int D, int lane) {
  float acc = 0.f;
  for (int q = lane; q < D / 4; q += 64) {
    const float4 u = reinterpret_cast<const float4*>(a)[q], v = reinterpret_cast<const float4*>(b)[q];
    acc = fmaf(u.x, v.x, acc); acc = fmaf(u.y, v.y, acc); acc = fmaf(u.z, v.z, acc); acc = fmaf(u.w, v.w, acc);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  return acc;
}

// probe_tile.h's block_sum_to behind a barrier (`red` may still be read), the sum handed to every thread; `red` is LDS of 257 doubles
__device__ __forceinline__ double block_sum_f64(double* red, double v, int tid) {
  __syncthreads();
  block_sum_to(red, v, tid, red + 256);
  __syncthreads();
  return red[256];
}

// xn[i] = |x_i|^2; one wave per row
__global__ __launch_bounds__(256) void kmeans_rownorm_kernel(const float* __restrict__ X, int N, int D, float* __restrict__ xn) {
  const int lane = threadIdx.x & 63;
  const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N) return;
  const float v = wave_dot(X + i * D, X + i * D, D, lane);
  if (lane == 0) xn[i] = v;
}

// hb[k] = -1/2 |c_k|^2 (Euclidean; summed in double in the lane order of a wave) or 0 (cosine); one wave per centre
__global__ __launch_bounds__(256) void kmeans_bias_kernel(const float* __restrict__ C, int K, int D, int metric, float* __restrict__ hb) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= K) return;
  double acc = 0.0;
  if (metric == PLIPMI_KMEANS_EUCLIDEAN)
    for (int d = lane; d < D; d += 64) { const double v = C[(size_t)k * D + d]; acc += v * v; }
  acc = wave_sum_f64(acc);
  if (lane == 0) hb[k] = (float)(-0.5 * acc);
}

// labels[i] = first arg-max_k (x_i . c_k + hb[k]), scores[i] = that maximum (scores may be nullptr).  changed != nullptr: the number of
// rows whose label differs from what `labels` held is ADDED to *changed.  grid.x workgroups walk the 32-row tiles.
template <int CT>
__global__ __launch_bounds__(kThreads) void kmeans_assign_kernel(const float* __restrict__ X, int N, int D, const float* __restrict__ C, int K,
                                                                 const float* __restrict__ hb, int32_t* __restrict__ labels,
                                                                 float* __restrict__ scores, int32_t* __restrict__ changed) {
  using T = ProbeTile<CT>;
  constexpr int Dp = T::Dp;
  constexpr bool kPrefetch = CT <= 8;                // wider rows: the registers hold one slice only
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ int nchanged;
  float* xs = lds;                                   // [32][Dp], swizzled
  float* zp = xs + kRows * Dp;                       // [4][32][16] partial scores

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int rc = tid & 15, rr = tid >> 4;
  const long ntiles = ((long)N + kRows - 1) / kRows;
  const int groups = (K + kGroup - 1) / kGroup;
  if (tid == 0) nchanged = 0;
  int mine_changed = 0;
  for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    T::direct(X, N, D, t * kRows, tid, xs);
    float4 wf[CT], wn[kPrefetch ? CT : 1];
    T::load_centres(wf, C, K, D, 0, wave, lane);
    __syncthreads();
    float best[2] = {-INFINITY, -INFINITY};
    int bk[2] = {0, 0};
    for (int g = 0; g < groups; ++g) {
      if constexpr (kPrefetch) {
        if (g + 1 < groups) T::load_centres(wn, C, K, D, (g + 1) * kGroup, wave, lane);
      }
      T::tile_scores(xs, wf, zp, wave, lane);
      __syncthreads();
      const int cls = g * kGroup + rc;
      if (cls < K) {
        const float bias = hb[cls];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int o = (rr + 16 * h) * kGroup + rc;
          const float z = join_scores(zp, o, bias);
          if (z > best[h]) { best[h] = z; bk[h] = cls; }      // groups ascend: an equal score keeps the lower k
        }
      }
      __syncthreads();
      if (g + 1 < groups) {
        if constexpr (kPrefetch) {
#pragma unroll
          for (int j = 0; j < CT; ++j) wf[j] = wn[j];
        } else {
          T::load_centres(wf, C, K, D, (g + 1) * kGroup, wave, lane);
        }
      }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {                    // the row's 16 columns: larger score, then lower k (every lane takes part)
      float b = best[h];
      int k = bk[h];
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) {
        const float ob = __shfl_xor(b, o, 16);
        const int ok = __shfl_xor(k, o, 16);
        if (ob > b || (ob == b && ok < k)) { b = ob; k = ok; }
      }
      const long gr = t * kRows + rr + 16 * h;
      if (rc == 0 && gr < N) {
        if (changed) mine_changed += labels[gr] != k;
        labels[gr] = k;
        if (scores) scores[gr] = b;
      }
    }
  }
  if (changed) {
    __syncthreads();
    if (mine_changed) atomicAdd(&nchanged, mine_changed);
    __syncthreads();
    if (tid == 0 && nchanged) atomicAdd(changed, nchanged);
  }
}

// ---- update ---------------------------------------------------------------------------------------------------------------------
// block b owns rows [b RB, (b + 1) RB): hist[b][k] = its rows of label k; ipart[b] = its rows' distances, summed in double (thread
// t adds rows t, t + 256, ..., the threads are added in thread order).  A label outside [0, K) belongs to no cluster.
__global__ __launch_bounds__(256) void kmeans_hist_kernel(const int32_t* __restrict__ labels, const float* __restrict__ scores,
                                                          const float* __restrict__ xn, int N, int K, int RB, int metric,
                                                          int32_t* __restrict__ hist, double* __restrict__ ipart) {
  extern __shared__ __attribute__((aligned(16))) int32_t hsh[];      // [K]
  __shared__ double red[257];
  const int tid = threadIdx.x, b = blockIdx.x;
  for (int k = tid; k < K; k += 256) hsh[k] = 0;
  __syncthreads();
  const long lo = (long)b * RB, hi = std::min<long>(N, lo + RB);
  double acc = 0.0;
  for (long i = lo + tid; i < hi; i += 256) {
    const int l = labels[i];
    if (l >= 0 && l < K) {
      atomicAdd(&hsh[l], 1);
      acc += (double)km_dist(metric, metric == PLIPMI_KMEANS_EUCLIDEAN ? xn[i] : 0.f, scores[i]);
    }
  }
  __syncthreads();
  for (int k = tid; k < K; k += 256) hist[(size_t)b * K + k] = hsh[k];
  const double s = block_sum_f64(red, acc, tid);
  if (tid == 0) ipart[b] = s;
}

// hist[b][k] -> the rows of label k in the blocks before b; counts[k] = all of them
__global__ __launch_bounds__(256) void kmeans_colscan_kernel(int32_t* __restrict__ hist, int nb, int K, int32_t* __restrict__ counts) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  int run = 0;
  for (int b = 0; b < nb; ++b) {
    const int v = hist[(size_t)b * K + k];
    hist[(size_t)b * K + k] = run;
    run += v;
  }
  counts[k] = run;
}

// ONE workgroup: offs[k] = the members of the clusters before k, choff[k] = their chunks (kChunk members each), both [K + 1]
__global__ __launch_bounds__(256) void kmeans_offsets_kernel(const int32_t* __restrict__ counts, int K, int32_t* __restrict__ offs,
                                                             int32_t* __restrict__ choff) {
  __shared__ int pm[256], pc[256];
  const int tid = threadIdx.x;
  const int per = (K + 255) / 256;
  const int lo = std::min(K, tid * per), hi = std::min(K, lo + per);
  int m = 0, c = 0;
  for (int k = lo; k < hi; ++k) { m += counts[k]; c += (counts[k] + kChunk - 1) / kChunk; }
  pm[tid] = m; pc[tid] = c;
  __syncthreads();
  if (tid == 0) {
    int am = 0, ac = 0;
    for (int i = 0; i < 256; ++i) { const int vm = pm[i], vc = pc[i]; pm[i] = am; pc[i] = ac; am += vm; ac += vc; }
    offs[K] = am; choff[K] = ac;
  }
  __syncthreads();
  m = pm[tid]; c = pc[tid];
  for (int k = lo; k < hi; ++k) { offs[k] = m; choff[k] = c; m += counts[k]; c += (counts[k] + kChunk - 1) / kChunk; }
}

// order[offs[k] + rank] = row, rank = the rows of label k below it: the blocks before (base), the 256-row batches before it in this
// block (run[k]) and the rows below it in its batch (counted).  Stable: every cluster's rows ascend.
__global__ __launch_bounds__(256) void kmeans_scatter_kernel(const int32_t* __restrict__ labels, int N, int K, int RB,
                                                             const int32_t* __restrict__ base, const int32_t* __restrict__ offs,
                                                             int32_t* __restrict__ order) {
  extern __shared__ __attribute__((aligned(16))) int32_t run[];      // [K]
  __shared__ int lab[256];
  const int tid = threadIdx.x, b = blockIdx.x;
  for (int k = tid; k < K; k += 256) run[k] = offs[k] + base[(size_t)b * K + k];
  __syncthreads();
  const long lo = (long)b * RB, hi = std::min<long>(N, lo + RB);
  for (long i0 = lo; i0 < hi; i0 += 256) {
    const long i = i0 + tid;
    int l = i < hi ? labels[i] : -1;
    if (l < 0 || l >= K) l = -1;
    lab[tid] = l;
    __syncthreads();
    int below = 0, all = 0;
    if (l >= 0) {
      for (int j = 0; j < 256; ++j) {
        const int same = lab[j] == l;
        all += same;
        below += same & (j < tid);
      }
      order[run[l] + below] = (int32_t)i;
    }
    __syncthreads();
    if (l >= 0 && below == all - 1) run[l] += all;      // the label's last row of the batch
    __syncthreads();
  }
}

// block g = chunk (g - choff[k]) of the cluster k that owns it: part[g][:] = its members' rows summed, prep[g] = its best member.
// Q = D / 4 column groups x S = 256 / Q slices; slice j adds members j, j + S, ... in ascending order, then the slices in slice order.
__global__ __launch_bounds__(256) void kmeans_chunk_kernel(const float* __restrict__ X, int D, const float* __restrict__ scores, int K,
                                                           const int32_t* __restrict__ order, const int32_t* __restrict__ offs,
                                                           const int32_t* __restrict__ choff, float* __restrict__ part,
                                                           int32_t* __restrict__ prep) {
  __shared__ float4 sl4[256];
  __shared__ float bs[4];
  __shared__ int br[4];
  const int tid = threadIdx.x, g = blockIdx.x;
  if (g >= choff[K]) return;
  int lo = 0, hi = K;                                // the k with choff[k] <= g < choff[k + 1]
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (choff[mid] <= g) lo = mid; else hi = mid; }
  const int k = lo;
  const int first = offs[k] + (g - choff[k]) * kChunk;
  const int cnt = std::min(kChunk, offs[k + 1] - first);
  const int Q = D / 4, S = 256 / Q;
  const int q = tid % Q, j0 = tid / Q;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (j0 < S)
    for (int j = j0; j < cnt; j += S) {
      const float4 v = reinterpret_cast<const float4*>(X + (size_t)order[first + j] * D)[q];
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
  sl4[tid] = acc;
  // the best member: larger score, then lower row
  float s = -INFINITY;
  int r = INT_MAX;
  if (tid < cnt) { r = order[first + tid]; s = scores[r]; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float os = __shfl_xor(s, o, 64);
    const int orow = __shfl_xor(r, o, 64);
    if (os > s || (os == s && orow < r)) { s = os; r = orow; }
  }
  if ((tid & 63) == 0) { bs[tid >> 6] = s; br[tid >> 6] = r; }
  __syncthreads();
  if (tid < Q) {
    float4 a = sl4[tid];
    for (int j = 1; j < S; ++j) { const float4 v = sl4[j * Q + tid]; a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }
    reinterpret_cast<float4*>(part + (size_t)g * D)[tid] = a;
  }
  if (tid == 0) {
    for (int w = 1; w < 4; ++w)
      if (bs[w] > s || (bs[w] == s && br[w] < r)) { s = bs[w]; r = br[w]; }
    prep[g] = r;
  }
}

// block k: sums[k][:] = its chunks' partial sums in chunk order (double, rounded once), reps[k] = the best of its chunks' best members
// (-1: empty).  Block 0 also sums the nb distance partials in block order -> *inertia.
__global__ __launch_bounds__(256) void kmeans_combine_kernel(const float* __restrict__ part, const int32_t* __restrict__ prep,
                                                             const float* __restrict__ scores, const int32_t* __restrict__ choff, int D,
                                                             const double* __restrict__ ipart, int nb, float* __restrict__ sums,
                                                             int32_t* __restrict__ reps, double* __restrict__ inertia) {
  const int tid = threadIdx.x, k = blockIdx.x;
  const int c0 = choff[k], c1 = choff[k + 1];
  for (int d = tid; d < D; d += 256) {
    double acc = 0.0;
    for (int c = c0; c < c1; ++c) acc += (double)part[(size_t)c * D + d];
    sums[(size_t)k * D + d] = (float)acc;
  }
  if (tid == 0) {
    int r = -1;
    float s = -INFINITY;
    for (int c = c0; c < c1; ++c) {
      const int cr = prep[c];
      const float cs = scores[cr];
      if (r < 0 || cs > s || (cs == s && cr < r)) { s = cs; r = cr; }
    }
    reps[k] = r;
  }
  if (k == 0 && tid == 64) {
    double acc = 0.0;
    for (int b = 0; b < nb; ++b) acc += ipart[b];
    *inertia = acc;
  }
}

// block k: the new centre of cluster k in place, shiftk[k] = |new - old|^2 in double, empty[k] = 1 (centre and shift untouched) when
// it has no member or -- cosine -- a zero sum
__global__ __launch_bounds__(256) void kmeans_finalise_kernel(const float* __restrict__ sums, const int32_t* __restrict__ counts, int D,
                                                              int metric, float* __restrict__ C, double* __restrict__ shiftk,
                                                              int32_t* __restrict__ empty) {
  __shared__ double red[257];
  const int tid = threadIdx.x, k = blockIdx.x;
  const int cnt = counts[k];
  double n2 = 0.0;
  if (metric == PLIPMI_KMEANS_COSINE) {
    double a = 0.0;
    for (int d = tid; d < D; d += 256) { const double v = sums[(size_t)k * D + d]; a += v * v; }
    n2 = block_sum_f64(red, a, tid);
  }
  if (cnt == 0 || (metric == PLIPMI_KMEANS_COSINE && !(n2 > 0.0))) {      // uniform over the block
    if (tid == 0) { empty[k] = 1; shiftk[k] = 0.0; }
    return;
  }
  const double nrm = sqrt(n2);
  double sh = 0.0;
  for (int d = tid; d < D; d += 256) {
    const float v = sums[(size_t)k * D + d];
    const float c = metric == PLIPMI_KMEANS_COSINE ? (float)((double)v / nrm) : v / (float)cnt;
    const double dl = (double)c - (double)C[(size_t)k * D + d];
    sh += dl * dl;
    C[(size_t)k * D + d] = c;
  }
  sh = block_sum_f64(red, sh, tid);
  if (tid == 0) { empty[k] = 0; shiftk[k] = sh; }
}

// ONE workgroup: st->shift = sum_k shiftk[k] (thread t adds k = t, t + 256, ..., the threads in thread order), st->n_empty, st->inertia
__global__ __launch_bounds__(256) void kmeans_status_kernel(const double* __restrict__ shiftk, const int32_t* __restrict__ empty, int K,
                                                            const double* __restrict__ inertia, KmStatus* __restrict__ st) {
  __shared__ double red[257];
  const int tid = threadIdx.x;
  double a = 0.0, e = 0.0;
  for (int k = tid; k < K; k += 256) { a += shiftk[k]; e += (double)empty[k]; }
  a = block_sum_f64(red, a, tid);
  e = block_sum_f64(red, e, tid);            // a count below 2^53: exact
  if (tid == 0) { st->shift = a; st->n_empty = (int32_t)e; st->inertia = *inertia; }
}

// ---- seeding --------------------------------------------------------------------------------------------------------------------
// block b owns rows [b RB, (b + 1) RB), RB % 256 == 0.  mind_i = min(mind_i, d(x_i, X[*pick])) (first: = d; a picked row: 0), then bsum[b] = its mind
// summed in double: thread t sums its run of RB / 256 consecutive rows, thread 0 adds the runs in order.
__global__ __launch_bounds__(256) void kmeans_seed_dist_kernel(const float* __restrict__ X, int N, int D, const float* __restrict__ xn,
                                                               int metric, const int32_t* __restrict__ pick,
                                                               const int32_t* __restrict__ taken, int first, int RB,
                                                               float* __restrict__ mind, double* __restrict__ bsum) {
  __shared__ double red[257];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, b = blockIdx.x;
  const long lo = (long)b * RB, hi = std::min<long>(N, lo + RB);
  const long p = *pick;
  const float* c = X + p * D;
  const float half_cn = 0.5f * xn[p];
  for (long i = lo + wave; i < hi; i += 4) {
    const float dot = wave_dot(X + i * D, c, D, lane);
    const float d = km_dist(metric, xn[i], metric == PLIPMI_KMEANS_EUCLIDEAN ? dot - half_cn : dot);
    if (lane == 0) mind[i] = taken[i] ? 0.f : (first ? d : fminf(mind[i], d));      // a picked row is never picked again
  }
  __syncthreads();                                   // this block's own stores, read back below
  const int per = RB / 256;
  double run = 0.0;
  for (long i = lo + (long)tid * per; i < std::min<long>(hi, lo + (long)(tid + 1) * per); ++i) run += (double)mind[i];
  const double s = block_sum_f64(red, run, tid);
  if (tid == 0) bsum[b] = s;
}

// ONE workgroup: pick t.  total = the block sums in order; the pick is the first row i with
//   P_block(b) + (P_run(r) + (mind of the run's rows up to i)) > u * total,
// the association kmeans_seed_dist_kernel summed in; total == 0 (or no such row, which rounding alone could cause): the lowest row not
// yet picked.  forced >= 0 (pick 0, which the host knows): that row, no search.  Then picks[t] = row, taken[row] = 1, mind[row] = 0,
// centers[t] = X[row].
__global__ __launch_bounds__(256) void kmeans_seed_pick_kernel(const float* __restrict__ X, int N, int D, float* __restrict__ mind,
                                                               const double* __restrict__ bsum, int nb, int RB, double u, int t,
                                                               int forced, int32_t* __restrict__ taken, int32_t* __restrict__ picks,
                                                               float* __restrict__ centers) {
  __shared__ double runs[256];
  __shared__ double pb, target;
  __shared__ int blk, row;
  const int tid = threadIdx.x;
  const int per = RB / 256;
  if (tid == 0) {
    blk = -1; row = forced;
    double total = 0.0;
    if (forced < 0)
      for (int b = 0; b < nb; ++b) total += bsum[b];
    target = u * total;
    if (total > 0.0) {
      double acc = 0.0;
      for (int b = 0; b < nb; ++b) {
        if (acc + bsum[b] > target) { blk = b; pb = acc; break; }
        acc += bsum[b];
      }
    }
  }
  __syncthreads();
  if (blk >= 0) {
    const long lo = (long)blk * RB, hi = std::min<long>(N, lo + RB);
    double run = 0.0;
    for (long i = lo + (long)tid * per; i < std::min<long>(hi, lo + (long)(tid + 1) * per); ++i) run += (double)mind[i];
    runs[tid] = run;
    __syncthreads();
    if (tid == 0) {
      double pr = 0.0;
      for (int r = 0; r < 256 && row < 0; ++r) {
        if (pb + (pr + runs[r]) > target) {
          double seq = 0.0;
          for (long i = lo + (long)r * per; i < std::min<long>(hi, lo + (long)(r + 1) * per); ++i) {
            seq += (double)mind[i];
            if (pb + (pr + seq) > target) { row = (int)i; break; }
          }
        }
        pr += runs[r];
      }
    }
  }
  if (tid == 0) {
    if (row < 0)
      for (int i = 0; i < N; ++i)
        if (!taken[i]) { row = i; break; }
    if (row < 0) row = 0;                            // K <= N: not reached
    picks[t] = row;
    taken[row] = 1;
    mind[row] = 0.f;
  }
  __syncthreads();
  const long r = row;
  for (int d = tid; d < D; d += 256) centers[(size_t)t * D + d] = X[r * D + d];
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// rows per block of the histogram / seeding passes (a multiple of 256), and the number of such blocks (at most 1024 from N = 2^20 on)
int km_block_rows(int N) { return (int)align_up(std::max<size_t>(1024, ((size_t)N + 1023) / 1024), 256); }
int km_blocks(int N) { return (N + km_block_rows(N) - 1) / km_block_rows(N); }
int km_max_chunks(int N, int K) { return (N + kChunk - 1) / kChunk + K; }

struct KmScratch {
  float *xn, *hb, *mind, *part, *sums, *scores;
  double *bsum, *ipart, *shiftk, *inertia;
  int32_t *taken, *picks, *order, *hist, *offs, *choff, *prep, *empty, *counts, *reps;
  KmStatus* status;
  size_t total;
};

KmScratch km_layout(char* base, int N, int D, int K) {
  Carver cv;
  cv.base = base;
  const size_t nb = km_blocks(N), G = km_max_chunks(N, K);
  KmScratch L;
  L.xn = cv.take<float>(N, 4);          L.hb = cv.take<float>(K, 4);            L.mind = cv.take<float>(N, 4);
  L.part = cv.take<float>(G * D, 4);    L.sums = cv.take<float>((size_t)K * D, 4); L.scores = cv.take<float>(N, 4);
  L.bsum = cv.take<double>(nb, 8);      L.ipart = cv.take<double>(nb, 8);       L.shiftk = cv.take<double>(K, 8);
  L.inertia = cv.take<double>(1, 8);
  L.taken = cv.take<int32_t>(N, 4);     L.picks = cv.take<int32_t>(K, 4);       L.order = cv.take<int32_t>(N, 4);
  L.hist = cv.take<int32_t>(nb * K, 4); L.offs = cv.take<int32_t>(K + 1, 4);    L.choff = cv.take<int32_t>(K + 1, 4);
  L.prep = cv.take<int32_t>(G, 4);      L.empty = cv.take<int32_t>(K, 4);       L.counts = cv.take<int32_t>(K, 4);
  L.reps = cv.take<int32_t>(K, 4);
  L.status = cv.take<KmStatus>(1, sizeof(KmStatus));
  L.total = align_up(cv.off, 256);
  return L;
}

int km_check(const char* who, plipmi_handle h, const void* X, int N, int D, int K, int metric) {
  if (!h) return fail(PLIPMI_ERR_INVALID, "%s: null handle", who);
  if (!X) return fail(PLIPMI_ERR_INVALID, "%s: null X", who);
  if (metric != PLIPMI_KMEANS_EUCLIDEAN && metric != PLIPMI_KMEANS_COSINE)
    return fail(PLIPMI_ERR_INVALID, "%s: unknown metric %d (0 = euclidean, 1 = cosine)", who, metric);
  RUN(check_embeddings((std::string(who) + ": ").c_str(), X, N, D));
  if (K < 1 || K > PLIPMI_KMEANS_MAX_K || K > N)
    return fail(PLIPMI_ERR_INVALID, "%s: need 1 <= K <= min(N, %d) clusters, got K = %d with N = %d", who, PLIPMI_KMEANS_MAX_K, K, N);
  return PLIPMI_OK;
}

int km_reserve(plipmi_handle h, int N, int D, int K, hipStream_t s, KmScratch* L) {
  RUN(h->kmeans_ws.reserve(km_layout(nullptr, N, D, K).total, s));
  *L = km_layout(h->kmeans_ws.data(), N, D, K);
  return PLIPMI_OK;
}

int km_rownorm(plipmi_handle h, const float* X, int N, int D, const KmScratch& L, hipStream_t s) {
  Scope sc(h, s, "kmeans_rownorm", 2.0 * N * (double)D, (double)N * D * 4);
  hipLaunchKernelGGL(kmeans_rownorm_kernel, dim3((N + 3) / 4), dim3(256), 0, s, X, N, D, L.xn);
  HIP_TRY(hipGetLastError());
  return PLIPMI_OK;
}

// the bias of the centres, then the assignment pass
int km_assign(plipmi_handle h, const float* X, int N, int D, const float* C, int K, int metric, const KmScratch& L, int32_t* labels,
              float* scores, int32_t* changed, hipStream_t s) {
  hipLaunchKernelGGL(kmeans_bias_kernel, dim3((K + 3) / 4), dim3(256), 0, s, C, K, D, metric, L.hb);
  HIP_TRY(hipGetLastError());
  const long ntiles = ((long)N + kRows - 1) / kRows;
  const int nwg = probe_stream_workgroups(N, D);
  Scope sc(h, s, "kmeans_assign", 2.0 * N * (double)D * K, (double)N * D * 4 + (double)nwg * ((ntiles + nwg - 1) / nwg) * K * D * 4);
  HIP_TRY(probe_dispatch(probe_col_tiles(D), [&](auto ct) -> hipError_t {
    constexpr int CT = decltype(ct)::value;
    const size_t lds = probe_lds_bytes(CT, 0);
    if (const hipError_t e = allow_lds<&kmeans_assign_kernel<CT>>(lds); e != hipSuccess) return e;
    kmeans_assign_kernel<CT><<<nwg, kThreads, lds, s>>>(X, N, D, C, K, L.hb, labels, scores, changed);
    return hipGetLastError();
  }));
  return PLIPMI_OK;
}

// the update step; L.xn must hold the row norms (Euclidean)
int km_update(plipmi_handle h, const float* X, int N, int D, const int32_t* labels, const float* scores, int K, int metric,
              const KmScratch& L, float* sums, int32_t* counts, int32_t* reps, double* inertia, hipStream_t s) {
  const int RB = km_block_rows(N), nb = km_blocks(N), G = km_max_chunks(N, K);
  Scope sc(h, s, "kmeans_update", (double)N * D, 2.0 * N * D * 4);
  hipLaunchKernelGGL(kmeans_hist_kernel, dim3(nb), dim3(256), (size_t)K * 4, s, labels, scores, (const float*)L.xn, N, K, RB, metric, L.hist,
                     L.ipart);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(kmeans_colscan_kernel, dim3((K + 255) / 256), dim3(256), 0, s, L.hist, nb, K, counts);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(kmeans_offsets_kernel, dim3(1), dim3(256), 0, s, (const int32_t*)counts, K, L.offs, L.choff);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(kmeans_scatter_kernel, dim3(nb), dim3(256), (size_t)K * 4, s, labels, N, K, RB, (const int32_t*)L.hist,
                     (const int32_t*)L.offs, L.order);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(kmeans_chunk_kernel, dim3(G), dim3(256), 0, s, X, D, scores, K, (const int32_t*)L.order, (const int32_t*)L.offs,
                     (const int32_t*)L.choff, L.part, L.prep);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(kmeans_combine_kernel, dim3(K), dim3(256), 0, s, (const float*)L.part, (const int32_t*)L.prep, scores,
                     (const int32_t*)L.choff, D, (const double*)L.ipart, nb, sums, reps, inertia);
  HIP_TRY(hipGetLastError());
  return PLIPMI_OK;
}

}  // namespace

}  // namespace plipmi

using namespace plipmi;

extern "C" {

int plipmi_kmeans_seed(plipmi_handle h, const float* X, int N, int D, int K, int metric, const double* u_host, float* centers,
                       int32_t* picks, void* stream) {
  RUN(km_check("plipmi_kmeans_seed", h, X, N, D, K, metric));
  if (!u_host || !centers) return fail(PLIPMI_ERR_INVALID, "plipmi_kmeans_seed: null u_host / centers");
  for (int t = 0; t < K; ++t)
    if (!(u_host[t] >= 0.0 && u_host[t] < 1.0)) return fail(PLIPMI_ERR_INVALID, "plipmi_kmeans_seed: u[%d] = %g is outside [0, 1)", t, u_host[t]);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  KmScratch L;
  RUN(km_reserve(h, N, D, K, s, &L));
  const int RB = km_block_rows(N), nb = km_blocks(N);
  RUN(km_rownorm(h, X, N, D, L, s));
  HIP_TRY(hipMemsetAsync(L.taken, 0, (size_t)N * 4, s));
  const int p0 = (int)std::min<long>(N - 1, (long)(u_host[0] * (double)N));
  Scope sc(h, s, "kmeans_seed", 2.0 * N * (double)D * (K - 1), (double)N * D * 4 * (K - 1));
  hipLaunchKernelGGL(kmeans_seed_pick_kernel, dim3(1), dim3(256), 0, s, X, N, D, L.mind, (const double*)L.bsum, nb, RB, 0.0, 0, p0, L.taken,
                     L.picks, centers);
  HIP_TRY(hipGetLastError());
  for (int t = 1; t < K; ++t) {
    hipLaunchKernelGGL(kmeans_seed_dist_kernel, dim3(nb), dim3(256), 0, s, X, N, D, (const float*)L.xn, metric, (const int32_t*)L.picks + (t - 1),
                       (const int32_t*)L.taken, t == 1 ? 1 : 0, RB, L.mind, L.bsum);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(kmeans_seed_pick_kernel, dim3(1), dim3(256), 0, s, X, N, D, L.mind, (const double*)L.bsum, nb, RB, u_host[t], t, -1, L.taken,
                       L.picks, centers);
    HIP_TRY(hipGetLastError());
  }
  if (picks) HIP_TRY(hipMemcpyAsync(picks, L.picks, (size_t)K * 4, hipMemcpyDeviceToDevice, s));
  return PLIPMI_OK;
}

int plipmi_kmeans_assign(plipmi_handle h, const float* X, int N, int D, const float* centers, int K, int metric, int32_t* labels,
                         float* scores, void* stream) {
  RUN(km_check("plipmi_kmeans_assign", h, X, N, D, K, metric));
  if (!centers || !labels) return fail(PLIPMI_ERR_INVALID, "plipmi_kmeans_assign: null centers / labels");
  if (reinterpret_cast<uintptr_t>(centers) % 16) return fail(PLIPMI_ERR_INVALID, "plipmi_kmeans_assign: centers must be 16-byte aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  KmScratch L;
  RUN(km_reserve(h, N, D, K, s, &L));
  return km_assign(h, X, N, D, centers, K, metric, L, labels, scores, nullptr, s);
}

int plipmi_kmeans_update(plipmi_handle h, const float* X, int N, int D, const int32_t* labels, const float* scores, int K, int metric,
                         float* sums, int32_t* counts, int32_t* reps, double* inertia, void* stream) {
  RUN(km_check("plipmi_kmeans_update", h, X, N, D, K, metric));
  if (!labels || !scores || !sums || !counts || !reps || !inertia)
    return fail(PLIPMI_ERR_INVALID, "plipmi_kmeans_update: null labels / scores / sums / counts / reps / inertia");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  KmScratch L;
  RUN(km_reserve(h, N, D, K, s, &L));
  if (metric == PLIPMI_KMEANS_EUCLIDEAN) RUN(km_rownorm(h, X, N, D, L, s));
  return km_update(h, X, N, D, labels, scores, K, metric, L, sums, counts, reps, inertia, s);
}

int plipmi_kmeans_fit(plipmi_handle h, const float* X, int N, int D, int K, int metric, int max_iter, double tol_abs,
                      float* centers_inout, int32_t* labels, float* scores, int32_t* counts, int32_t* reps, plipmi_kmeans_info* info,
                      void* stream) {
  RUN(km_check("plipmi_kmeans_fit", h, X, N, D, K, metric));
  if (!centers_inout || !labels) return fail(PLIPMI_ERR_INVALID, "plipmi_kmeans_fit: null centers_inout / labels");
  if (reinterpret_cast<uintptr_t>(centers_inout) % 16) return fail(PLIPMI_ERR_INVALID, "plipmi_kmeans_fit: centers_inout must be 16-byte aligned");
  if (max_iter < 1 || !(tol_abs >= 0.0)) return fail(PLIPMI_ERR_INVALID, "plipmi_kmeans_fit: need max_iter >= 1 and tol_abs >= 0");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  KmScratch L;
  RUN(km_reserve(h, N, D, K, s, &L));
  RUN(h->kmeans_host.reserve(256 + align_up((size_t)K * 4, 256) + 2 * align_up((size_t)N * 4, 256), s));
  KmStatus* st_h = reinterpret_cast<KmStatus*>(h->kmeans_host.data());
  int32_t* empty_h = reinterpret_cast<int32_t*>(h->kmeans_host.data() + 256);
  float* sc_h = reinterpret_cast<float*>(h->kmeans_host.data() + 256 + align_up((size_t)K * 4, 256));
  float* xn_h = sc_h + align_up((size_t)N * 4, 256) / 4;
  float* sc = scores ? scores : L.scores;
  int32_t* cn = counts ? counts : L.counts;
  int32_t* rp = reps ? reps : L.reps;

  if (metric == PLIPMI_KMEANS_EUCLIDEAN) RUN(km_rownorm(h, X, N, D, L, s));
  HIP_TRY(hipMemsetAsync(labels, 0xFF, (size_t)N * 4, s));      // -1: every label of the first pass counts as changed
  int iters = 0, relocations = 0;
  bool strict = false, converged = false;
  double shift = 0.0, inertia = 0.0;
  std::vector<char> taken;
  for (int it = 0; it < max_iter; ++it) {
    HIP_TRY(hipMemsetAsync(&L.status->changed, 0, 4, s));
    RUN(km_assign(h, X, N, D, centers_inout, K, metric, L, labels, sc, &L.status->changed, s));
    RUN(km_update(h, X, N, D, labels, sc, K, metric, L, L.sums, cn, rp, L.inertia, s));
    hipLaunchKernelGGL(kmeans_finalise_kernel, dim3(K), dim3(256), 0, s, (const float*)L.sums, (const int32_t*)cn, D, metric, centers_inout,
                       L.shiftk, L.empty);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(kmeans_status_kernel, dim3(1), dim3(256), 0, s, (const double*)L.shiftk, (const int32_t*)L.empty, K,
                       (const double*)L.inertia, L.status);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(st_h, L.status, sizeof(KmStatus), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    iters = it + 1;
    shift = st_h->shift;
    inertia = st_h->inertia;
    if (st_h->n_empty > 0) {
      // the rare path: the distances of this iteration's assignment on the host, one row per empty cluster in ascending k
      HIP_TRY(hipMemcpyAsync(empty_h, L.empty, (size_t)K * 4, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipMemcpyAsync(sc_h, sc, (size_t)N * 4, hipMemcpyDeviceToHost, s));
      if (metric == PLIPMI_KMEANS_EUCLIDEAN) HIP_TRY(hipMemcpyAsync(xn_h, L.xn, (size_t)N * 4, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      taken.assign(N, 0);
      for (int k = 0; k < K; ++k) {
        if (!empty_h[k]) continue;
        int best = -1;
        float bd = 0.f;
        for (int i = 0; i < N; ++i) {
          if (taken[i]) continue;
          const float d = metric == PLIPMI_KMEANS_EUCLIDEAN ? fmaxf(0.f, xn_h[i] - 2.f * sc_h[i]) : fmaxf(0.f, 1.f - sc_h[i]);
          if (best < 0 || d > bd) { best = i; bd = d; }
        }
        taken[best] = 1;          // K <= N: a row is always left
        HIP_TRY(hipMemcpyAsync(centers_inout + (size_t)k * D, X + (size_t)best * D, (size_t)D * 4, hipMemcpyDeviceToDevice, s));
        ++relocations;
      }
      continue;                   // an iteration that moved a centre does not stop the loop
    }
    if (st_h->changed == 0) { strict = converged = true; break; }
    if (shift <= tol_abs) { converged = true; break; }
  }
  if (!strict) {                  // the labels on the device belong to the centres of the last update's input: one more pass
    RUN(km_assign(h, X, N, D, centers_inout, K, metric, L, labels, sc, nullptr, s));
    RUN(km_update(h, X, N, D, labels, sc, K, metric, L, L.sums, cn, rp, L.inertia, s));
    HIP_TRY(hipMemcpyAsync(&st_h->inertia, L.inertia, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    inertia = st_h->inertia;
  }
  if (info) {
    memset(info, 0, sizeof(*info));
    info->iterations = iters; info->converged = converged ? 1 : 0; info->relocations = relocations;
    info->inertia = inertia; info->center_shift = shift;
  }
  return PLIPMI_OK;
}

}  // extern "C"
