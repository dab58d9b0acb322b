// bags.hip -- slide-level heads on cached embeddings X [N, D] fp32 whose rows are grouped in BAGS (contiguous row ranges given by
// offsets int32 [S + 1]): the entries of include/plipmi.h "bags of embeddings" and their kernels.  One unit behind everything that existed
// (build.py BAG_SOURCES): no other unit calls into it and no other unit's code changes.  The tile, the class rows' 16-byte operand form
// (ProbeTile load_centres / tile_scores), join_scores, the LDS byte count and the streaming workgroup count are probe_tile.h's; the
// X / N / D check is handle.h's check_embeddings.  The definition is tests/bags_common.py's numpy oracle; this file is its restatement.
//
//   offsets      bag_offsets_kernel: ONE workgroup copies offsets to the workspace, clamped to [0, N] and made non-decreasing (a running
//                maximum).  Every other kernel reads that copy only, so no row index leaves [0, N) whatever the caller's array holds.
//   scores       bag_score_kernel<CT>: the walk of kmeans_assign_kernel -- probe_tile.h's 32-row tile of X in swizzled LDS (X is read
//                ONCE), the class rows streamed past in groups of 16, exact-fp32 MFMA products, the four waves' partials joined in wave
//                order -- which writes scale * z to scoresT[c][i] instead of keeping a best column.  The 16 x 32 block of a group is
//                turned in LDS so that a wave stores two runs of 32 consecutive rows.  A row's bits depend on the row and T alone.
//   pieces       The row axis is cut into chunks of kBagChunk rows; a PIECE is bag ^ chunk.  Slot p < nch is the piece that starts at row
//                p * kBagChunk (void when a bag starts exactly there, or no bag holds that row); slot nch + b is the first piece of
//                bag b (void when the bag is empty).  A piece is found from its slot by one binary search: there is no table, no host
//                work per bag, and the grid is a function of N, S, C alone.
//   top-K        bag_piece_kernel, one workgroup per (slot, class): the piece's scores -> LDS as 64-bit words (order-preserving uint32 key
//                of the score, -0 as +0, NaN as -inf) << 32 | ~row, so that DESCENDING word order is "larger score first, equal scores:
//                lower row first"; a bitonic sort of the next power of two; a piece that is a whole bag is finished at once, any other
//                leaves its first KP = pow2(kmax) words in the workspace.  bag_merge_kernel, one workgroup per (chunk, class): the bag
//                that starts in the chunk and runs past its end takes its pieces' lists in row order, each by one bitonic merge that
//                keeps the first KP words, and is finished.  Selection is EXACT: a bag's first m words are among its pieces' first m.
//   finish       top_idx from the words; the float64 prefix sums rank by rank in one lane (the oracle's association: a pooled value is
//                the oracle's bit for bit given the scores); pooled = (float)(sum / m).  bag_pred_kernel: one lane per (bag, k) takes
//                the first arg-max over the classes.
//   mean         bag_mean_piece_kernel / bag_mean_merge_kernel: the same pieces; a piece's column sums in float64 (slice j of the threads
//                adds rows j, j + SL, ... in ascending order, the slices are added in slice order), a bag's pieces added in row order.
//
// No floating-point atomics, no atomics at all; every sum has a fixed order: the same inputs give the same bits on every run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>

#include "handle.h"
#include "probe_tile.h"

namespace plipmi {

namespace {

constexpr int kBagChunk = 2048;      // rows per chunk: a piece is at most this long (>= PLIPMI_BAG_MAX_K, a power of two)
constexpr int kBagMeanCols = 1024;   // doubles per slot of the mean's partial sums (the widest D)
constexpr int kScoreTurn = kGroup * (kRows + 1);   // floats of the score kernel's 16 x 32 turn buffer (rows padded to 33)

struct BagKs { int32_t n, k[PLIPMI_BAG_MAX_KS]; };

struct BagPiece { int bag, lo, hi, slot; bool whole; };

// the order-preserving image of a score: a ranks before b as floats <=> key(a) > key(b); -0 is +0, a NaN is -inf
__device__ __forceinline__ uint32_t bag_key(float f) {
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) u = 0xff800000u;
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// back to the score as fp64, subnormals by integer arithmetic (exact whatever the fp32 denormal mode is)
__device__ __forceinline__ double bag_key_value(uint32_t k) {
  const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  const uint32_t mag = u & 0x7fffffffu;
  const double v = (mag >> 23) == 0 ? (double)(int)mag * 0x1p-149 : (double)__uint_as_float(mag);
  return (u & 0x80000000u) ? -v : v;
}
__device__ __forceinline__ int bag_word_row(uint64_t w) { return (int)(0xffffffffu - (uint32_t)w); }

// the last b in [0, S) with off[b] <= row, or -1 (off is the clean copy: non-decreasing, inside [0, N])
__device__ __forceinline__ int bag_of_row(const int32_t* __restrict__ off, int S, int row) {
  if (off[0] > row) return -1;
  int lo = 0, hi = S;
  while (hi - lo > 1) { const int mid = lo + ((hi - lo) >> 1); if (off[mid] <= row) lo = mid; else hi = mid; }
  return lo;
}

// slot p -> its piece; false: the slot is void.  *empty_bag = a bag slot whose bag has no rows.
__device__ __forceinline__ bool bag_piece(const int32_t* __restrict__ off, int S, int nch, long p, BagPiece* q, bool* empty_bag) {
  *empty_bag = false;
  if (p < nch) {
    const int row = (int)p * kBagChunk;
    const int b = bag_of_row(off, S, row);
    if (b < 0 || off[b] == row || row >= off[b + 1]) return false;
    q->bag = b; q->lo = row; q->hi = (int)std::min<long>(off[b + 1], (long)row + kBagChunk); q->slot = (int)p; q->whole = false;
    return true;
  }
  const int b = (int)(p - nch);
  const int lo = off[b], e = off[b + 1];
  q->bag = b;
  if (e <= lo) { *empty_bag = true; return false; }
  q->lo = lo; q->hi = (int)std::min<long>(e, ((long)lo / kBagChunk + 1) * kBagChunk); q->slot = nch + lo / kBagChunk; q->whole = q->hi == e;
  return true;
}

// the bag that starts in chunk c0 and runs past its end, or -1
__device__ __forceinline__ int bag_crossing(const int32_t* __restrict__ off, int S, int N, int c0) {
  const long rb = ((long)c0 + 1) * kBagChunk;
  if (rb >= N) return -1;
  const int b = bag_of_row(off, S, (int)rb - 1);
  if (b < 0 || off[b + 1] <= rb || off[b] < (long)c0 * kBagChunk) return -1;
  return b;
}

__global__ __launch_bounds__(256) void bag_offsets_kernel(const int32_t* __restrict__ offsets, int S, int N, int32_t* __restrict__ off) {
  __shared__ int pm[256];
  const int tid = threadIdx.x;
  const long per = ((long)S + 1 + 255) / 256;         // thread t owns entries [t per, (t + 1) per)
  const long lo = std::min<long>((long)S + 1, tid * per), hi = std::min<long>((long)S + 1, lo + per);
  int m = 0;
  for (long i = lo; i < hi; ++i) m = std::max(m, std::min(std::max(offsets[i], 0), N));
  pm[tid] = m;
  __syncthreads();
  int run = 0;
  for (int i = 0; i < tid; ++i) run = std::max(run, pm[i]);
  for (long i = lo; i < hi; ++i) { run = std::max(run, std::min(std::max(offsets[i], 0), N)); off[i] = run; }
}

// scoresT[c][i] = scale * (x_i . t_c), c < C <= 64, class-major with leading dimension ld >= N.  grid.x workgroups walk the 32-row tiles.
template <int CT>
__global__ __launch_bounds__(kThreads) void bag_score_kernel(const float* __restrict__ X, int N, int D, const float* __restrict__ T, int C,
                                                             float scale, float* __restrict__ scoresT, long ld) {
  using PT = ProbeTile<CT>;
  constexpr int Dp = PT::Dp;
  constexpr bool kPrefetch = CT <= 8;                // wider rows: the registers hold one slice only
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xs = lds;                                   // [32][Dp], swizzled
  float* zp = xs + kRows * Dp;                       // [4][32][16] partial scores
  float* zt = zp + 4 * kRows * kGroup;               // [16][33] one group's scores, class-major

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int rc = tid & 15, rr = tid >> 4;
  const int sr = tid & 31, scl = tid >> 5;           // the store's row and class (and class + 8)
  const long ntiles = ((long)N + kRows - 1) / kRows;
  const int groups = (C + kGroup - 1) / kGroup;
  for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    PT::direct(X, N, D, t * kRows, tid, xs);
    float4 wf[CT], wn[kPrefetch ? CT : 1];
    PT::load_centres(wf, T, C, D, 0, wave, lane);
    __syncthreads();
    for (int g = 0; g < groups; ++g) {
      if constexpr (kPrefetch) {
        if (g + 1 < groups) PT::load_centres(wn, T, C, D, (g + 1) * kGroup, wave, lane);
      }
      PT::tile_scores(xs, wf, zp, wave, lane);
      __syncthreads();                               // zp is whole; the previous group's zt has been stored
#pragma unroll
      for (int h = 0; h < 2; ++h) zt[rc * (kRows + 1) + rr + 16 * h] = scale * join_scores(zp, (rr + 16 * h) * kGroup + rc, 0.f);
      __syncthreads();
      const long gr = t * kRows + sr;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int cls = g * kGroup + scl + 8 * h;
        if (gr < N && cls < C) scoresT[(long)cls * ld + gr] = zt[(scl + 8 * h) * (kRows + 1) + sr];
      }
      if (g + 1 < groups) {
        if constexpr (kPrefetch) {
#pragma unroll
          for (int j = 0; j < CT; ++j) wf[j] = wn[j];
        } else {
          PT::load_centres(wf, T, C, D, (g + 1) * kGroup, wave, lane);
        }
      }
    }
  }
}

// ---- top-K pooling ----------------------------------------------------------------------------------------------------------------
// (bag b, class c) from its first m = min(kmax, n) words, descending in w[]: top_idx (may be nullptr) and pooled
__device__ __forceinline__ void bag_finish(const uint64_t* w, int n, int b, int c, int C, int kmax, const BagKs& ks,
                                           float* __restrict__ pooled, int32_t* __restrict__ top_idx, int tid) {
  const int m = std::min(kmax, n);
  if (top_idx)
    for (int r = tid; r < kmax; r += 256) top_idx[((size_t)b * C + c) * kmax + r] = r < m ? bag_word_row(w[r]) : -1;
  if (tid == 0) {                                    // one lane, rank by rank: the oracle's association
    double acc = 0.0;
    int e = 0;
    for (int j = 0; j < ks.n; ++j) {
      const int mj = std::min(ks.k[j], n);
      for (; e < mj; ++e) acc += bag_key_value((uint32_t)(w[e] >> 32));
      pooled[((size_t)b * ks.n + j) * C + c] = (float)(acc / (double)mj);
    }
  }
}

// grid (nch + S, C).  scoresT [C][ld]; lists u64 [2 nch][C][KP]
__global__ __launch_bounds__(256) void bag_piece_kernel(const float* __restrict__ scoresT, long ld, int N, int C, const int32_t* __restrict__ off,
                                                        int S, int nch, int kmax, int KP, BagKs ks, uint64_t* __restrict__ lists,
                                                        float* __restrict__ pooled, int32_t* __restrict__ top_idx) {
  __shared__ uint64_t w[kBagChunk];
  const int tid = threadIdx.x, c = blockIdx.y;
  BagPiece q;
  bool empty_bag;
  if (!bag_piece(off, S, nch, blockIdx.x, &q, &empty_bag)) {
    if (empty_bag) {                                 // uniform over the block
      if (top_idx)
        for (int r = tid; r < kmax; r += 256) top_idx[((size_t)q.bag * C + c) * kmax + r] = -1;
      if (tid < ks.n) pooled[((size_t)q.bag * ks.n + tid) * C + c] = __uint_as_float(0x7fc00000u);
    }
    return;
  }
  const int len = q.hi - q.lo;
  int n2 = 2;
  while (n2 < len) n2 <<= 1;
  const float* src = scoresT + (long)c * ld + q.lo;
  for (int i = tid; i < n2; i += 256)
    w[i] = i < len ? ((uint64_t)bag_key(src[i]) << 32) | (uint64_t)(0xffffffffu - (uint32_t)(q.lo + i)) : 0ull;   // 0: behind every score
  __syncthreads();
  for (int k = 2; k <= n2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < n2 / 2; t += 256) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const uint64_t a = w[i], b = w[l];
        if ((a < b) == ((i & k) == 0)) { w[i] = b; w[l] = a; }
      }
      __syncthreads();
    }
  if (q.whole) {
    bag_finish(w, len, q.bag, c, C, kmax, ks, pooled, top_idx, tid);
    return;
  }
  uint64_t* dst = lists + ((size_t)q.slot * C + c) * KP;
  for (int r = tid; r < KP; r += 256) dst[r] = r < n2 ? w[r] : 0ull;
}

// grid (nch, C): the bag that starts in chunk blockIdx.x and runs past its end
__global__ __launch_bounds__(256) void bag_merge_kernel(int N, int C, const int32_t* __restrict__ off, int S, int nch, int kmax, int KP, BagKs ks,
                                                        const uint64_t* __restrict__ lists, float* __restrict__ pooled,
                                                        int32_t* __restrict__ top_idx) {
  __shared__ uint64_t w[2 * PLIPMI_BAG_MAX_K];
  const int tid = threadIdx.x, c = blockIdx.y, c0 = blockIdx.x;
  const int b = bag_crossing(off, S, N, c0);
  if (b < 0) return;
  const int end = off[b + 1];
  const uint64_t* first = lists + ((size_t)(nch + c0) * C + c) * KP;
  for (int r = tid; r < KP; r += 256) w[r] = first[r];
  for (int p = c0 + 1; p < nch && (long)p * kBagChunk < end; ++p) {
    const uint64_t* nxt = lists + ((size_t)p * C + c) * KP;
    for (int r = tid; r < KP; r += 256) w[KP + r] = nxt[KP - 1 - r];      // descending, then ascending: bitonic
    __syncthreads();
    for (int j = KP; j > 0; j >>= 1) {
      for (int t = tid; t < KP; t += 256) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const uint64_t a = w[i], v = w[l];
        if (a < v) { w[i] = v; w[l] = a; }
      }
      __syncthreads();
    }
  }
  __syncthreads();
  bag_finish(w, end - off[b], b, c, C, kmax, ks, pooled, top_idx, tid);
}

// one lane per (bag, k): the first arg-max over the classes (a NaN never wins over a number); an empty bag gives -1
__global__ __launch_bounds__(256) void bag_pred_kernel(const float* __restrict__ pooled, const int32_t* __restrict__ off, int S, int nks, int C,
                                                       int32_t* __restrict__ pred) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)S * nks) return;
  const int b = (int)(i / nks);
  if (off[b + 1] <= off[b]) { pred[i] = -1; return; }
  const float* row = pooled + i * C;
  float best = row[0];
  int bc = 0;
  for (int c = 1; c < C; ++c) {
    const float v = row[c];
    if (v > best || (best != best && v == v)) { best = v; bc = c; }
  }
  pred[i] = bc;
}

// ---- bag mean ---------------------------------------------------------------------------------------------------------------------
// mrow (LDS, D floats) = the bag's mean rounded to fp32 -> out[D]; normalize: divided by its norm (float64 sum of squares: thread t adds
// columns t, t + 256, ..., the threads are added in thread order), zeros for a zero norm.  red is LDS of 257 doubles.
__device__ __forceinline__ void bag_mean_finish(const float* mrow, double* red, int D, int normalize, float* __restrict__ out, int tid) {
  __syncthreads();
  double nrm = 1.0;
  if (normalize) {
    double a = 0.0;
    for (int d = tid; d < D; d += 256) { const double v = mrow[d]; a += v * v; }
    block_sum_to(red, a, tid, red + 256);
    __syncthreads();
    nrm = sqrt(red[256]);
  }
  for (int d = tid; d < D; d += 256) out[d] = normalize ? (nrm > 0.0 ? (float)((double)mrow[d] / nrm) : 0.f) : mrow[d];
}

// grid (nch + S).  part double [2 nch][kBagMeanCols]
__global__ __launch_bounds__(256) void bag_mean_piece_kernel(const float* __restrict__ X, int D, const int32_t* __restrict__ off, int S, int nch,
                                                             int normalize, double* __restrict__ part, float* __restrict__ mean) {
  __shared__ double sl[256][4];
  __shared__ double red[257];
  __shared__ float mrow[kBagMeanCols];
  const int tid = threadIdx.x;
  BagPiece q;
  bool empty_bag;
  if (!bag_piece(off, S, nch, blockIdx.x, &q, &empty_bag)) {
    if (empty_bag)
      for (int d = tid; d < D; d += 256) mean[(size_t)q.bag * D + d] = 0.f;
    return;
  }
  const int Q = D / 4, SL = 256 / Q;
  const int qc = tid % Q, j0 = tid / Q;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  if (j0 < SL)
    for (long r = (long)q.lo + j0; r < q.hi; r += SL) {
      const float4 v = reinterpret_cast<const float4*>(X + r * D)[qc];
      a0 += (double)v.x; a1 += (double)v.y; a2 += (double)v.z; a3 += (double)v.w;
    }
  sl[tid][0] = a0; sl[tid][1] = a1; sl[tid][2] = a2; sl[tid][3] = a3;
  __syncthreads();
  if (tid < Q) {
    for (int j = 1; j < SL; ++j) { a0 += sl[j * Q + tid][0]; a1 += sl[j * Q + tid][1]; a2 += sl[j * Q + tid][2]; a3 += sl[j * Q + tid][3]; }
    if (q.whole) {
      const double n = (double)(q.hi - q.lo);
      mrow[4 * tid] = (float)(a0 / n); mrow[4 * tid + 1] = (float)(a1 / n); mrow[4 * tid + 2] = (float)(a2 / n); mrow[4 * tid + 3] = (float)(a3 / n);
    } else {
      double* dst = part + (size_t)q.slot * kBagMeanCols + 4 * tid;
      dst[0] = a0; dst[1] = a1; dst[2] = a2; dst[3] = a3;
    }
  }
  if (q.whole) bag_mean_finish(mrow, red, D, normalize, mean + (size_t)q.bag * D, tid);      // uniform over the block
}

// grid (nch): the bag that starts in chunk blockIdx.x and runs past its end
__global__ __launch_bounds__(256) void bag_mean_merge_kernel(int N, int D, const int32_t* __restrict__ off, int S, int nch, int normalize,
                                                             const double* __restrict__ part, float* __restrict__ mean) {
  __shared__ double red[257];
  __shared__ float mrow[kBagMeanCols];
  const int tid = threadIdx.x, c0 = blockIdx.x;
  const int b = bag_crossing(off, S, N, c0);
  if (b < 0) return;
  const int end = off[b + 1];
  const double n = (double)(end - off[b]);
  for (int d = tid; d < D; d += 256) {
    double acc = part[(size_t)(nch + c0) * kBagMeanCols + d];
    for (int p = c0 + 1; p < nch && (long)p * kBagChunk < end; ++p) acc += part[(size_t)p * kBagMeanCols + d];
    mrow[d] = (float)(acc / n);
  }
  bag_mean_finish(mrow, red, D, normalize, mean + (size_t)b * D, tid);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
int bag_chunks(int N) { return (int)(((long)N + kBagChunk - 1) / kBagChunk); }
int bag_pow2(int k) { int p = 2; while (p < k) p <<= 1; return p; }

struct BagScratch {
  int32_t* off;
  uint64_t* lists;
  float* scores;
  double* part;
  size_t total;
};

BagScratch bag_layout(char* base, int N, int S, int C, int kmax) {
  Carver cv;
  cv.base = base;
  const size_t nch = bag_chunks(N);
  BagScratch L;
  L.off = cv.take<int32_t>((size_t)S + 1, 4);
  L.lists = cv.take<uint64_t>(2 * nch * C * bag_pow2(kmax), 8);
  L.scores = cv.take<float>((size_t)C * N, 4);
  L.part = cv.take<double>(2 * nch * kBagMeanCols, 8);
  L.total = align_up(cv.off, 256);
  return L;
}

bool bag_sizes_ok(int N, int S, int C, int kmax) {
  return N >= 1 && S >= 1 && C >= 1 && C <= PLIPMI_BAG_MAX_CLASSES && kmax >= 1 && kmax <= PLIPMI_BAG_MAX_K;
}

int bag_check_ks(const char* who, const int32_t* ks_host, int nks, BagKs* ks) {
  if (!ks_host) return fail(PLIPMI_ERR_INVALID, "%s: null ks_host", who);
  if (nks < 1 || nks > PLIPMI_BAG_MAX_KS) return fail(PLIPMI_ERR_INVALID, "%s: need 1 <= nks <= %d values of k, got %d", who, PLIPMI_BAG_MAX_KS, nks);
  ks->n = nks;
  for (int j = 0; j < PLIPMI_BAG_MAX_KS; ++j) ks->k[j] = 0;
  for (int j = 0; j < nks; ++j) {
    if (ks_host[j] < 1 || ks_host[j] > PLIPMI_BAG_MAX_K)
      return fail(PLIPMI_ERR_INVALID, "%s: ks[%d] = %d is outside 1 .. %d", who, j, ks_host[j], PLIPMI_BAG_MAX_K);
    if (j && ks_host[j] <= ks_host[j - 1]) return fail(PLIPMI_ERR_INVALID, "%s: ks must be strictly ascending, got ks[%d] = %d after %d", who, j, ks_host[j], ks_host[j - 1]);
    ks->k[j] = ks_host[j];
  }
  return PLIPMI_OK;
}

int bag_check_common(const char* who, plipmi_handle h, const int32_t* offsets, int S, int C, const void* workspace) {
  if (!h) return fail(PLIPMI_ERR_INVALID, "%s: null handle", who);
  if (!offsets || !workspace) return fail(PLIPMI_ERR_INVALID, "%s: null offsets / workspace", who);
  if (S < 1) return fail(PLIPMI_ERR_INVALID, "%s: need S >= 1 bags, got %d", who, S);
  if (C < 1 || C > PLIPMI_BAG_MAX_CLASSES) return fail(PLIPMI_ERR_INVALID, "%s: need 1 <= C <= %d classes, got %d", who, PLIPMI_BAG_MAX_CLASSES, C);
  if (reinterpret_cast<uintptr_t>(workspace) % 16) return fail(PLIPMI_ERR_INVALID, "%s: workspace must be 16-byte aligned", who);
  return PLIPMI_OK;
}

int bag_clean_offsets(const int32_t* offsets, int S, int N, const BagScratch& L, hipStream_t s) {
  hipLaunchKernelGGL(bag_offsets_kernel, dim3(1), dim3(256), 0, s, offsets, S, N, L.off);
  HIP_TRY(hipGetLastError());
  return PLIPMI_OK;
}

// pieces, merges, predictions; L.off holds the clean offsets
int bag_pool(plipmi_handle h, const float* scoresT, long ld, int N, int C, int S, const BagKs& ks, const BagScratch& L, float* pooled,
             int32_t* pred, int32_t* top_idx, hipStream_t s) {
  const int nch = bag_chunks(N), kmax = ks.k[ks.n - 1], KP = bag_pow2(kmax);
  Scope sc(h, s, "bag_pool", 0.0, (double)N * C * 4 + (double)S * C * (ks.n + (top_idx ? kmax : 0)) * 4);
  hipLaunchKernelGGL(bag_piece_kernel, dim3((unsigned)(nch + (long)S), C), dim3(256), 0, s, scoresT, ld, N, C, (const int32_t*)L.off, S, nch, kmax,
                     KP, ks, L.lists, pooled, top_idx);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(bag_merge_kernel, dim3(nch, C), dim3(256), 0, s, N, C, (const int32_t*)L.off, S, nch, kmax, KP, ks,
                     (const uint64_t*)L.lists, pooled, top_idx);
  HIP_TRY(hipGetLastError());
  if (pred) {
    hipLaunchKernelGGL(bag_pred_kernel, dim3((unsigned)(((long)S * ks.n + 255) / 256)), dim3(256), 0, s, (const float*)pooled,
                       (const int32_t*)L.off, S, ks.n, C, pred);
    HIP_TRY(hipGetLastError());
  }
  return PLIPMI_OK;
}

}  // namespace

}  // namespace plipmi

using namespace plipmi;

extern "C" {

size_t plipmi_bag_workspace(int N, int S, int C, int kmax) {
  if (!bag_sizes_ok(N, S, C, kmax)) return 0;
  return bag_layout(nullptr, N, S, C, kmax).total;
}

int plipmi_bag_pool_scores(plipmi_handle h, const float* scoresT, int64_t ld, int N, int C, const int32_t* offsets, int S,
                           const int32_t* ks_host, int nks, void* workspace, float* pooled, int32_t* pred, int32_t* top_idx, void* stream) {
  const char* who = "plipmi_bag_pool_scores";
  RUN(bag_check_common(who, h, offsets, S, C, workspace));
  if (!scoresT || !pooled) return fail(PLIPMI_ERR_INVALID, "%s: null scoresT / pooled", who);
  if (N < 1) return fail(PLIPMI_ERR_INVALID, "%s: need N > 0 rows, got %d", who, N);
  if (ld < N) return fail(PLIPMI_ERR_INVALID, "%s: need ld >= N, got ld = %lld with N = %d", who, (long long)ld, N);
  BagKs ks;
  RUN(bag_check_ks(who, ks_host, nks, &ks));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const BagScratch L = bag_layout(static_cast<char*>(workspace), N, S, C, ks.k[nks - 1]);
  RUN(bag_clean_offsets(offsets, S, N, L, s));
  return bag_pool(h, scoresT, (long)ld, N, C, S, ks, L, pooled, pred, top_idx, s);
}

int plipmi_bag_topk_pool(plipmi_handle h, const float* X, int N, int D, const int32_t* offsets, int S, const float* T, int C, float scale,
                         const int32_t* ks_host, int nks, void* workspace, float* pooled, int32_t* pred, int32_t* top_idx,
                         float* scores_out, void* stream) {
  const char* who = "plipmi_bag_topk_pool";
  RUN(bag_check_common(who, h, offsets, S, C, workspace));
  if (!X || !T || !pooled) return fail(PLIPMI_ERR_INVALID, "%s: null X / T / pooled", who);
  RUN(check_embeddings("plipmi_bag_topk_pool: ", X, N, D));
  if (reinterpret_cast<uintptr_t>(T) % 16) return fail(PLIPMI_ERR_INVALID, "%s: T must be 16-byte aligned", who);
  BagKs ks;
  RUN(bag_check_ks(who, ks_host, nks, &ks));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const BagScratch L = bag_layout(static_cast<char*>(workspace), N, S, C, ks.k[nks - 1]);
  RUN(bag_clean_offsets(offsets, S, N, L, s));
  float* sc = scores_out ? scores_out : L.scores;
  {
    const long ntiles = ((long)N + kRows - 1) / kRows;
    const int nwg = probe_stream_workgroups(N, D);
    Scope scope(h, s, "bag_scores", 2.0 * N * (double)D * C,
                (double)N * D * 4 + (double)nwg * ((ntiles + nwg - 1) / nwg) * C * D * 4 + (double)N * C * 4);
    HIP_TRY(probe_dispatch(probe_col_tiles(D), [&](auto ct) -> hipError_t {
      constexpr int CT = decltype(ct)::value;
      const size_t lds = probe_lds_bytes(CT, kScoreTurn);
      if (const hipError_t e = allow_lds<&bag_score_kernel<CT>>(lds); e != hipSuccess) return e;
      bag_score_kernel<CT><<<nwg, kThreads, lds, s>>>(X, N, D, T, C, scale, sc, (long)N);
      return hipGetLastError();
    }));
  }
  return bag_pool(h, sc, (long)N, N, C, S, ks, L, pooled, pred, top_idx, s);
}

int plipmi_bag_mean(plipmi_handle h, const float* X, int N, int D, const int32_t* offsets, int S, int normalize, void* workspace, float* mean,
                    void* stream) {
  const char* who = "plipmi_bag_mean";
  RUN(bag_check_common(who, h, offsets, S, 1, workspace));
  if (!X || !mean) return fail(PLIPMI_ERR_INVALID, "%s: null X / mean", who);
  RUN(check_embeddings("plipmi_bag_mean: ", X, N, D));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const BagScratch L = bag_layout(static_cast<char*>(workspace), N, S, 1, 1);
  RUN(bag_clean_offsets(offsets, S, N, L, s));
  const int nch = bag_chunks(N);
  Scope sc(h, s, "bag_mean", (double)N * D, (double)N * D * 4 + (double)S * D * 4);
  hipLaunchKernelGGL(bag_mean_piece_kernel, dim3((unsigned)(nch + (long)S)), dim3(256), 0, s, X, D, (const int32_t*)L.off, S, nch, normalize ? 1 : 0,
                     L.part, mean);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(bag_mean_merge_kernel, dim3(nch), dim3(256), 0, s, N, D, (const int32_t*)L.off, S, nch, normalize ? 1 : 0,
                     (const double*)L.part, mean);
  HIP_TRY(hipGetLastError());
  return PLIPMI_OK;
}

}  // extern "C"
