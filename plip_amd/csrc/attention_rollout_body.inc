// attention_rollout_body.inc -- the BODY of the rollout step kernel, included between the braces of a __global__ function
// (both in attention_summary.hip: head 64, and the padded sizes that carry heads of 72 .. 128).  Text, not a function: as
// an inlined function template the head-64 kernels came out with other instructions than before the head became a parameter (the
// same arithmetic); included as text they are the same instructions (profiles/head_dim_isa_diff.txt).  The including kernel provides
//   T, RPL               the element type of qkv; tile rows per lane in the score phase and in the product (score_tile)
//   qkv, R_in, R_out, S, H, causal, key_mask, row_idx, pooled_out   its arguments
//   constexpr int DP     columns of a staged q row: kDh, or the padded size 96 / 128
//   head                 the head's columns: kDh as a constant at head 64, else the kernel's argument
// and `using namespace probs_dev`.  grid (row tiles, B); dynamic LDS: rollout_lds_bytes(S, DP).
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int S4 = (S + 3) & ~3;
  float* qs = lds;                       // [kRows][DP]
  float* ab = qs + kRows * DP;           // [kRows][S4]: the head sum, then A^ (columns S .. S4: zeros)
  float* sc = ab + kRows * S4;           // [kRows][S]
  const int i0 = blockIdx.x * kRows, b = blockIdx.y;
  const int D = H * head, ld = 3 * D;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int rows = min(kRows, S - i0);
  // the tile that holds the pooled row also stores P[b, h][pooled row, :] (fp32 [B, H, S]): pooled_r = its tile row there, else -1
  const int pooled_r = pooled_out ? min(max(row_idx[b], 0), S - 1) - i0 : -1;
  float* pooled_b = (pooled_r >= 0 && pooled_r < kRows) ? pooled_out + (size_t)b * H * S : nullptr;

  for (int e = tid; e < kRows * S4; e += kThreads) ab[e] = 0.f;
  for (int h = 0; h < H; ++h) {
    const T* base = qkv + (size_t)b * S * ld + h * head;
    stage_q<T, kRows, DP>(qs, base, ld, i0, rows, tid, head);
    __syncthreads();
    score_tile<T, kRows, RPL, DP>(qs, sc, base, ld, D, S, i0, rows, b, causal, key_mask, tid, head);
    __syncthreads();
    for (int r = wave; r < rows; r += kThreads / 64) {     // row r is wave r % 4's in every head: no two waves touch one row of ab
      float* ar = ab + r * S4;
      float* pr = (pooled_b && r == pooled_r) ? pooled_b + (size_t)h * S : nullptr;
      softmax_row_in_place(sc + r * S, S, lane, [ar, pr](int j, float p) {
#pragma clang fp contract(off)      // the sum of the probabilities as stored: p is rounded before it is added
        ar[j] = ar[j] + p;
        if (pr) pr[j] = p;
      });
    }
    __syncthreads();
  }

  // A^ = (1/2) (A / H) + (1/2) I
  const float half_mean = 0.5f / (float)H;
  for (int e = tid; e < kRows * S4; e += kThreads) {
    const int r = e / S4, k = e - r * S4;
    const float a = ab[e] * half_mean;
    ab[e] = (r < rows && k == i0 + r) ? a + 0.5f : a;
  }
  __syncthreads();

  constexpr int kLanes = kThreads / (kRows / RPL);
  const int r0 = (tid / kLanes) * RPL;
  float* out = R_out + ((size_t)b * S + i0) * S;
  if (R_in == nullptr) {
    for (int c = tid % kLanes; c < S; c += kLanes)
#pragma unroll
      for (int r = 0; r < RPL; ++r)
        if (r0 + r < rows) out[(size_t)(r0 + r) * S + c] = ab[(r0 + r) * S4 + c];
    return;
  }
  const float* Rb = R_in + (size_t)b * S * S;
  for (int c = tid % kLanes; c < S; c += kLanes) {
    float acc[RPL];
#pragma unroll
    for (int r = 0; r < RPL; ++r) acc[r] = 0.f;
    int k = 0;
    for (; k + 3 < S; k += 4) {
      const float x0 = Rb[(size_t)k * S + c], x1 = Rb[(size_t)(k + 1) * S + c], x2 = Rb[(size_t)(k + 2) * S + c],
                  x3 = Rb[(size_t)(k + 3) * S + c];
#pragma unroll
      for (int r = 0; r < RPL; ++r) {
        const float4 a = *reinterpret_cast<const float4*>(&ab[(r0 + r) * S4 + k]);
        acc[r] = fmaf(a.x, x0, acc[r]);
        acc[r] = fmaf(a.y, x1, acc[r]);
        acc[r] = fmaf(a.z, x2, acc[r]);
        acc[r] = fmaf(a.w, x3, acc[r]);
      }
    }
    for (; k < S; ++k) {
      const float x = Rb[(size_t)k * S + c];
#pragma unroll
      for (int r = 0; r < RPL; ++r) acc[r] = fmaf(ab[(r0 + r) * S4 + k], x, acc[r]);
    }
#pragma unroll
    for (int r = 0; r < RPL; ++r)
      if (r0 + r < rows) out[(size_t)(r0 + r) * S + c] = acc[r];
  }
