// attention_valu_body.inc -- the BODY of the exact-fp32 VALU attention kernel, included between the braces of a __global__ function
// (both in attention.hip: head 64, the kernel it has always been, and the padded sizes that carry heads of 72 .. 128).
// Text, not a function: as an inlined function template the head-64 kernels came out with other operand orders and register
// assignments than before the head became a parameter (the same arithmetic, other instructions); included as text they are the
// same instructions (profiles/head_dim_isa_diff.txt).  The including kernel provides
//   T                    the element type of qkv / out
//   qkv, out, S, H, causal, key_mask   its arguments
//   constexpr int DP     columns held per lane: 64, or the padded size 96 / 128
//   constexpr int KT     keys staged in LDS per step, a multiple of 8 (2 x KT x DP x 4 bytes of LDS)
//   head                 the head's columns: DP itself as a constant at 64, else the kernel's argument (head <= DP, head % 8 == 0)
// One query row per lane with the row's q and its accumulator in registers (DP each), K / V tiles of KT keys broadcast from LDS,
// flash-style online softmax in chunks of 8 keys.  At a padded size the columns past `head` of q, K and V are ZEROS (written, never
// read from memory): they add exact zeros to every score and their accumulators are never stored.
  constexpr bool kPadded = DP != 64;   // head < DP is possible: guard the loads and the store
  __shared__ __attribute__((aligned(16))) float Ks[KT][DP];
  __shared__ __attribute__((aligned(16))) float Vs[KT][DP];
  __shared__ int Mk[KT];

  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int D = H * head, ld = 3 * D;
  const int tid = threadIdx.x, nthreads = blockDim.x;
  const int i = tid;                       // query row of this lane
  const int ic = i < S ? i : S - 1;        // clamped (lanes past S compute a duplicate, never store)
  const int wave_last = min(S - 1, (__builtin_amdgcn_readfirstlane(tid >> 6)) * 64 + 63);
  const T* base = qkv + (size_t)b * S * ld + h * head;

  float q[DP], acc[DP];
  {
    const T* qr = base + (size_t)ic * ld;
#pragma unroll
    for (int d = 0; d < DP; d += 4) {
      const float4 t = (!kPadded || d < head) ? load4(qr + d) : make_float4(0.f, 0.f, 0.f, 0.f);
      q[d] = t.x; q[d + 1] = t.y; q[d + 2] = t.z; q[d + 3] = t.w;
    }
  }
#pragma unroll
  for (int d = 0; d < DP; ++d) acc[d] = 0.f;
  float m = -INFINITY, l = 0.f;

  // keys needed by anyone in the block: all of them, or up to the last row under the causal mask
  const int keys_block = S;
  for (int j0 = 0; j0 < keys_block; j0 += KT) {
    __syncthreads();  // previous tile fully consumed
    for (int e = tid; e < KT * (DP / 4); e += nthreads) {
      const int j = e / (DP / 4), d = (e - j * (DP / 4)) * 4;
      const int jg = min(j0 + j, S - 1);
      const T* kr = base + (size_t)jg * ld + D + d;
      if (!kPadded || d < head) {
        *reinterpret_cast<float4*>(&Ks[j][d]) = load4(kr);
        *reinterpret_cast<float4*>(&Vs[j][d]) = load4(kr + D);
      } else {
        *reinterpret_cast<float4*>(&Ks[j][d]) = make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4*>(&Vs[j][d]) = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    for (int j = tid; j < KT; j += nthreads) {
      const int jg = j0 + j;
      Mk[j] = (jg < S) && (key_mask == nullptr || key_mask[(size_t)b * S + jg] != 0);
    }
    __syncthreads();

    // wave-uniform number of keys of this tile that any row of this wave may attend to
    int nk = min(KT, S - j0);
    if (causal) nk = min(nk, wave_last - j0 + 1);
    for (int c0 = 0; c0 < nk; c0 += 8) {
      float s[8];
      float cmax = -INFINITY;
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        const int j = c0 + jj;  // < KT always (nk <= KT and tiles are KT rows, KT % 8 == 0)
        const float4* kr = reinterpret_cast<const float4*>(&Ks[j][0]);
        float a = 0.f;
#pragma unroll
        for (int d4 = 0; d4 < DP / 4; ++d4) {
          const float4 kv = kr[d4];
          a = fmaf(q[4 * d4 + 0], kv.x, a);
          a = fmaf(q[4 * d4 + 1], kv.y, a);
          a = fmaf(q[4 * d4 + 2], kv.z, a);
          a = fmaf(q[4 * d4 + 3], kv.w, a);
        }
        const bool ok = Mk[j] && (!causal || (j0 + j) <= i);
        s[jj] = ok ? a : -INFINITY;
        cmax = fmaxf(cmax, s[jj]);
      }
      const float m_new = fmaxf(m, cmax);
      const float m_use = (m_new == -INFINITY) ? 0.f : m_new;  // everything masked so far: keep zeros
      const float corr = expf(m - m_use);
      m = m_new;
      l *= corr;
#pragma unroll
      for (int d = 0; d < DP; ++d) acc[d] *= corr;
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        const float p = expf(s[jj] - m_use);
        l += p;
        const float4* vr = reinterpret_cast<const float4*>(&Vs[c0 + jj][0]);
#pragma unroll
        for (int d4 = 0; d4 < DP / 4; ++d4) {
          const float4 vv = vr[d4];
          acc[4 * d4 + 0] = fmaf(p, vv.x, acc[4 * d4 + 0]);
          acc[4 * d4 + 1] = fmaf(p, vv.y, acc[4 * d4 + 1]);
          acc[4 * d4 + 2] = fmaf(p, vv.z, acc[4 * d4 + 2]);
          acc[4 * d4 + 3] = fmaf(p, vv.w, acc[4 * d4 + 3]);
        }
      }
    }
  }
  if (i < S) {
    const float inv = 1.0f / l;
    T* orow = out + ((size_t)b * S + i) * D + h * head;
#pragma unroll
    for (int d = 0; d < DP; d += 4)
      if (!kPadded || d < head) store4(orow + d, acc[d] * inv, acc[d + 1] * inv, acc[d + 2] * inv, acc[d + 3] * inv);
  }
