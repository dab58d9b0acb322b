// attention_flash_step.inc -- the online-softmax step of the chunked MFMA attention kernels (attention_mfma.hip:
// attention_flash_kernel, head 64, and attention_flash_hd_kernel, the padded sizes that carry heads of 72 .. 128), included inside
// the chunk loop once a chunk's K / V images are staged and the barrier behind them is passed.  Text, not a function: helpers that
// held these loops changed the kernels' instructions (profiles/attention_shared_isa.txt, profiles/head_dim_isa_diff.txt); included
// as text the head-64 kernel is the instructions it was (profiles/head_hd_fold_isa_diff.txt).  Staging, barriers, the Q source,
// where the validity words come from and the output epilogue stay with each kernel.  The including kernel provides
//   HT, X8               the operand type and its 8-vector (half_traits<HT>::x8)
//   constexpr int NKS    k-steps of the score product: 4 at head 64, DP / 16 at a padded size
//   constexpr int NDT    32-column output tiles: 2, or DP / 32
//   constexpr int KPL    bytes between the 64-column planes of the K image (k-step ks reads plane ks >> 2 at step ks & 3; at four
//                        k-steps the term is 0)
//   constexpr int VIMG   bytes between the [keys][32 columns] V images
//   Ks, vlane            the K image; the lane's address in the first V image (vtr_lane_offset)
//   mhalf[2]             key validity (sequence end and key_mask) of the chunk's two 64-key halves, one bit per key
//   qf[NKS], acc[NDT], m_run, l_run    the Q fragments and the running state of the lane's query (l_run: this lane's half of the row sum)
//   S, causal, kbase, qbase, q0, qidx, lrow, hi, lsw
// Two 64-key halves per staged chunk: 32 score registers live instead of 64, one online-softmax update per half.
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      if (kbase + 64 * hf >= S) break;                           // wave-uniform: past the sequence end
      if (causal && kbase + 64 * hf > qbase + q0 + 31) break;  // wave-uniform: the rest is above the diagonal
      f32x16 sc[2];
      float cmax = -INFINITY;
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        const int t = 2 * hf + tt;
        const bool live = kbase + 32 * t < S && !(causal && kbase + 32 * t > qbase + q0 + 31);  // wave-uniform
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[tt][r] = 0.f;
        if (live) {
#pragma unroll
          for (int ks = 0; ks < NKS; ++ks)
            mma16<HT>(sc[tt], image_fragment(Ks + (ks >> 2) * KPL, 32 * t + lrow, ks & 3, hi, lsw), qf[ks]);
        }
        unsigned bits = live ? (unsigned)(mhalf[hf] >> (32 * tt)) : 0u;   // the keys this lane may use: validity AND causal limit
        if (causal) {
          const int d = qidx - (kbase + 32 * t);   // causal_bits(d), written out: the call changes the head-64 kernel's instructions
          bits &= d < 0 ? 0u : (d >= 31 ? 0xffffffffu : (2u << d) - 1u);
        }
        // every key of the tile usable by every query of the wave (the common case away from the sequence end and the
        // diagonal): no masking arithmetic at all
        if (__ballot(bits != 0xffffffffu) == 0ull) max_scores(sc[tt], cmax);
        else mask_scores(sc[tt], bits, hi, cmax);
      }
      cmax = fmaxf(cmax, __shfl_xor(cmax, 32, 64));
      const float m_new = fmaxf(m_run, cmax);
      const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
      const float m2 = m_use * kLog2e;
      const bool moved = m_new != m_run;    // (NaN-free: -inf != -inf is false, a first finite maximum is a move)
      // a lane whose maximum did not move rescales by EXACTLY 1 -- exp2 of the FMA's rounding residual is 1 +- 3e-6, and l_run
      // (always rescaled) would otherwise drift against acc (rescaled only when some lane moved): ADVICE r4
      const float scale = !moved ? 1.f : (m_run == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(fmaf(m_run, kLog2e, -m2));  // acc, l_run are 0 while m_run = -inf
      m_run = m_new;
      if (__ballot(moved) != 0ull) {        // wave-uniform: once the running maxima have settled the rescaling multiplies go
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[dt][r] *= scale;
      }
      float csum = 0.f;
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        const int t = 2 * hf + tt;
        if (kbase + 32 * t >= S || (causal && kbase + 32 * t > qbase + q0 + 31)) continue;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          X8 pf;
#pragma unroll
          for (int jj = 0; jj < 8; ++jj) {
            const float pv = __builtin_amdgcn_exp2f(fmaf(sc[tt][8 * s2 + jj], kLog2e, -m2));   // exp(x - m): one FMA + v_exp_f32
            csum += pv;
            pf[jj] = (HT)pv;
          }
#pragma unroll
          for (int dt = 0; dt < NDT; ++dt) acc[dt] = pv_step<HT>(vlane, VIMG, dt, 32 * t + 16 * s2, pf, acc[dt]);
        }
      }
      l_run = l_run * scale + csum;
    }
