// gemm_kernel.h -- the NT GEMM kernel that carries >98 % of the PLIP forward's FLOPs (interface: gemm.h).
//
//   C = epilogue( A[M,K] * W[N,K]^T )         A, W row-major, K contiguous
//
// which is exactly nn.Linear (HF stores Linear weights [out,in]) -- q/k/v, out_proj,
// fc1, fc2 (modeling_clip.py:293-296,343-344), the unfolded patch-embed conv
// (:148-154) and, with A = image embeds / W = text embeds, the logits (:814).
//
// gfx950 design
//   * MFMA: v_mfma_f32_16x16x32_bf16 / _f16 in the production tiles of the two 16-bit engines (variants 2, 3, 6: less
//     power per FLOP than 32x32x16, see the note above the kernel), v_mfma_f32_32x32x16 in the other 16-bit tiles, or
//     v_mfma_f32_32x32x2_f32 (exact fp32, fmaf-chain numerics).  Operands are SWAPPED -- the weight
//     fragment is the MFMA "A" operand and the activation fragment the "B"
//     operand -- so a lane ends up with 4 CONSECUTIVE output columns of one
//     output row per accumulator quad: 16-byte fp32 / 8-byte bf16 epilogue stores
//     and a float4 bias load instead of 2-byte scalar stores.
//   * LDS tile rows are always 128 bytes (BK = 64 bf16 / 32 fp32) = eight 16-byte
//     chunks; chunk c of row r lives at slot c ^ ((r>>1)&7).  With that XOR every
//     ds_read_b128 lane group (MI355X_MICROARCH LDS table) touches 16 distinct
//     16-byte slots of the 256-byte bank row: conflict-free fragment reads.
//   * global -> LDS staging through LDS-DMA (`buffer_load_dwordx4 ... lds`, or `global_load_lds_dwordx4` for
//     operands of 4 GiB and more): the LDS image is lane-linear, so the swizzle is applied to the per-lane SOURCE address.
//   * two LDS stages (one tile of lookahead) or, where three fit in the 160 KB (the 160x256 tile), a ring of three
//     (two tiles of lookahead, counted vmcnt); one barrier per K tile either way.  With operands resident in the
//     Infinity Cache the two are equal; with operands coming from HBM -- how the engine's kernels find the activations
//     the previous kernel wrote -- the second tile of lookahead is what covers the longer fill (profiles/r03_gemm_cold.txt).
//   * blockIdx -> tile map is XCD-aware: hardware round-robins blocks over the 8
//     XCDs, so block b is given logical tile (b%8)*ceil(n/8)+b/8 (bijective form)
//     and each XCD's private L2 sees a contiguous strip of M tiles sweeping N.
//
// Layout of the GEMM headers:
//   gemm.h           the interface (epilogue kinds, GemmParams, host entry points); no device code
//   gemm_lds.h       LDS-DMA, write-through store and MFMA helpers, shared with gemm_skinny.hip and qkv_attention.hip
//   gemm_tile.h      GemmTile: every compile-time quantity of an instantiation and its static_asserts; the notes on SCHED / NSTAGE / ADDR
//   gemm_fill.h      helpers of the staged fill and of the gather (im2col on load)
//   gemm_epilogue.h  EpilogueOp and the column-wise finishing arithmetic
//   this file        gemm_nt_kernel: tile assignment, staging (fill, gather), fragment helpers of each MFMA form, the K loop of the form
//                    in use (one `if constexpr` chain: ring of three / streamed 16x16x32 / two-stage 32x32), the epilogues.
// The kernel stays ONE function body on purpose: tools/isa_diff.py showed that moving a K loop, an epilogue or the fill into a function
// or a lambda of its own (state in a context struct or captured by reference) changes the instruction order and register allocation
// of every instantiation (profiles/gemm_split_isa.txt).  Inside the body each form's state and code exist only where
// `if constexpr` selects them.
#pragma once
#include "gemm_epilogue.h"
#include "gemm_fill.h"
#include "gemm_tile.h"

namespace plipmi {

// Publish the K tile that has been landing: this wave's pieces of it have arrived (ring of three: `counted` = a younger tile's LEAVE
// requests may stay in flight, vmcnt retires in order) and its last LDS reads of the tile before have returned; then the barrier.
template <int LEAVE>
__device__ __forceinline__ void publish_tile(bool counted) {
  if (counted) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LEAVE) : "memory");
  else wait_vm0();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __syncthreads();
}

// waves per SIMD the kernel is built for: 2 (LDS caps residency there, so let the allocator use 256 VGPRs)
template <typename T, int BM, int BN, int WM, int WN, int EPI, int SCHED = 0, int ADDR = 0, int NSTAGE = 2>
__global__ __launch_bounds__(WM* WN * 64) __attribute__((amdgpu_waves_per_eu(2, 2)))
void gemm_nt_kernel(const GemmParams p) {
  using TT = GemmTile<T, BM, BN, WM, WN, EPI, SCHED, ADDR, NSTAGE>;
  using OutT = typename TT::OutT;
  constexpr int NT = TT::NT, RB = TT::RB, MI = TT::MI, NI = TT::NI, TM = TT::TM, TN = TT::TN, MI2 = TT::MI2, NI2 = TT::NI2;
  constexpr int ELEMS16 = TT::ELEMS16, BK = TT::BK, A_BYTES = TT::A_BYTES, STAGE = TT::STAGE;
  constexpr int PA = TT::PA, PW = TT::PW, PA_MIN = TT::PA_MIN, NAL = TT::NAL;
  constexpr bool kHalf = TT::kHalf, kUneven = TT::kUneven, kSpread = TT::kSpread, kM16 = TT::kM16, kGather = TT::kGather,
                 kGatherU8 = TT::kGatherU8, kRowOperand = TT::kRowOperand;
  constexpr int kAddBufs = TT::kAddBufs, SLAB_PITCH = TT::SLAB_PITCH, SLAB_BYTES = TT::SLAB_BYTES;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int mi_w = kUneven ? (RB - wm * MI < MI ? RB - wm * MI : MI) : MI;   // this wave's 32-row blocks (wave-uniform)
  auto a_piece = [&](int i) -> bool {      // does this wave own A piece i of a tile?
    return PA == PA_MIN || i < PA_MIN || i * (NT / 8) + wave * 8 < BM;
  };

  // ---- XCD-aware tile assignment (bijective for any block count) -------------
  const int nbn = p.N / BN;
  const int nbm = (p.M + BM - 1) / BM;
  const int nblk = nbm * nbn;
  const int bid = blockIdx.x;
  const int xcd = bid & 7, xi = bid >> 3, xq = nblk >> 3, xr = nblk & 7;
  const int lid = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + xi;
  const int gw = p.gw > 0 ? p.gw : nbn, tpg = nbm * gw;  // column group width, tiles per group
  const int cgrp = lid / tpg, crem = lid - cgrp * tpg;
  const int m0 = (crem / gw) * BM, n0 = (cgrp * gw + crem % gw) * BN;
  int Mrt = p.M;   // live rows
  if (p.m_dev) {
    const int md = __builtin_amdgcn_readfirstlane(*p.m_dev);
    Mrt = md < p.M ? md : p.M;
    if (m0 >= Mrt) return;   // workgroup-uniform
  }

  // ---- staging addresses --------------------------------------------------
  // thread -> LDS chunk position q = pass*NT + tid: row = q>>3, slot = q&7, and the
  // K chunk that belongs in that slot is slot ^ ((row>>1)&7) (pass-independent).
  const int srow = tid >> 3;
  const int schunk = (tid & 7) ^ ((srow >> 1) & 7);
  const char* a_src[PA ? PA : 1];
  const char* w_src[PW];
#pragma unroll
  for (int i = 0; i < PA; ++i) {
    int r = m0 + i * (NT / 8) + srow;
    r = r < Mrt ? r : Mrt - 1;  // M edge: re-read the last row, stores are masked
    a_src[i] = reinterpret_cast<const char*>(p.A) + ((size_t)r * p.lda + schunk * ELEMS16) * sizeof(T);
  }
#pragma unroll
  for (int i = 0; i < PW; ++i) {
    const int r = n0 + i * (NT / 8) + srow;
    w_src[i] = reinterpret_cast<const char*>(p.W) + ((size_t)r * p.ldw + schunk * ELEMS16) * sizeof(T);
  }
  const unsigned lds0 =
      __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem);
  i32x4 rs_a, rs_w;
  unsigned a_off[PA ? PA : 1], w_off[PW];
  if constexpr (ADDR >= 1) {
    rs_a = make_buffer_rsrc(p.A);
    rs_w = make_buffer_rsrc(p.W);
#pragma unroll
    for (int i = 0; i < PA; ++i) a_off[i] = (unsigned)(a_src[i] - reinterpret_cast<const char*>(p.A));
#pragma unroll
    for (int i = 0; i < PW; ++i) w_off[i] = (unsigned)(w_src[i] - reinterpret_cast<const char*>(p.W));
  }
  unsigned koff = 0;  // ADDR 1: K byte offset of the tile being fetched (SGPR); advanced when its last piece is out
  auto dma_a = [&](int i, unsigned lds) {
    if (!a_piece(i)) return;
    if constexpr (ADDR >= 1) glds16_buf(rs_a, a_off[i], koff, lds);
    else { glds16(a_src[i], lds); a_src[i] += 128; }
  };
  auto dma_w = [&](int i, unsigned lds) {
    if constexpr (ADDR >= 1) glds16_buf(rs_w, w_off[i], koff, lds);
    else { glds16(w_src[i], lds); w_src[i] += 128; }
    if constexpr (ADDR >= 1) { if (i == PW - 1) koff += 128; }  // W pieces follow the A pieces: PW-1 is a tile's last
  };

  auto stage_issue = [&](int buf) {  // the whole tile at once; reads a_src/w_src (koff), then advances them by one K tile
    const unsigned base = lds0 + buf * STAGE + wave * 1024;
#pragma unroll
    for (int i = 0; i < PA; ++i) dma_a(i, base + i * NT * 16);
#pragma unroll
    for (int i = 0; i < PW; ++i) dma_w(i, base + A_BYTES + i * NT * 16);
  };
  // The same fill cut in kFillParts parts, one per K step that carries one, so that the requests do not queue on the texture-address
  // unit all at once and the last one has most of the iteration -- not a quarter of it -- to land before the end-of-iteration wait.
  // There are TWO mechanisms because they issue a tile's requests in a different order, and that order is part of the schedule:
  //   stage_issue_part (SCHED 6, the 32x32 burst schedule): part k in front of K step k's MFMA group;
  //   fill_batched / fill_part_placed (SCHED 7 / 8, the hand-placed K steps): below.
  // Both name a piece of the tile by its index (A pieces first): resource, lane offset and (compile-time) LDS offset.
  constexpr int kFillParts = 3;
  auto piece_rs = [&](int idx) __attribute__((always_inline)) -> const i32x4& { return idx < PA ? rs_a : rs_w; };
  auto piece_vo = [&](int idx) __attribute__((always_inline)) { return idx < PA ? a_off[idx < PA ? idx : 0] : w_off[idx >= PA && idx < PA + PW ? idx - PA : 0]; };
  constexpr auto piece_lds = [](int idx) constexpr { return idx < PA ? idx * NT * 16 : A_BYTES + (idx - PA) * NT * 16; };
  auto stage_issue_part = [&](int buf, int part) {
    const unsigned base = lds0 + buf * STAGE + wave * 1024;
    if constexpr (SCHED != 6) {
      // (the hand-placed schedules issue through fill_part_placed below)
    } else if constexpr (ADDR >= 1 && PA == PA_MIN) {
      constexpr int PER = (PA + PW + kFillParts - 1) / kFillParts;
      auto go = [&](auto part_c) {
        constexpr int P0 = decltype(part_c)::value * PER;
        constexpr int N = (P0 + PER <= PA + PW) ? PER : (PA + PW - P0 > 0 ? PA + PW - P0 : 0);
        if constexpr (N > 0) {
          constexpr int I0 = P0, I1 = P0 + (N > 1 ? 1 : 0), I2 = P0 + (N > 2 ? 2 : 0), I3 = P0 + (N > 3 ? 3 : 0);
          glds16_buf_n<N, piece_lds(I0), piece_lds(I1), piece_lds(I2), piece_lds(I3)>(
              base, koff, piece_rs(I0), piece_vo(I0), piece_rs(I1), piece_vo(I1), piece_rs(I2), piece_vo(I2), piece_rs(I3), piece_vo(I3));
          if constexpr (P0 + N == PA + PW) koff += 128;
        }
      };
      static_assert(PER <= 4, "glds16_buf_n batches at most four pieces");
      if (part == 0) go(std::integral_constant<int, 0>{});
      else if (part == 1) go(std::integral_constant<int, 1>{});
      else if (part == 2) go(std::integral_constant<int, 2>{});
      return;
    } else if constexpr (ADDR >= 1) {
      // partial last A pass: part 0 = this wave's A pieces (2 or 3 single requests), the W pieces split over the other parts
      static_assert(PW % 2 == 0 && PW <= 8, "W pieces are batched in two halves");
      constexpr int HW = PW / 2;
      auto w_half = [&](auto first_c) __attribute__((always_inline)) {   // HW consecutive W pieces from piece index first_c
        constexpr int I0 = decltype(first_c)::value, I1 = I0 + (HW > 1 ? 1 : 0), I2 = I0 + (HW > 2 ? 2 : 0), I3 = I0 + (HW > 3 ? 3 : 0);
        glds16_buf_n<HW, piece_lds(I0), piece_lds(I1), piece_lds(I2), piece_lds(I3)>(
            base, koff, piece_rs(I0), piece_vo(I0), piece_rs(I1), piece_vo(I1), piece_rs(I2), piece_vo(I2), piece_rs(I3), piece_vo(I3));
      };
      if (part == 0) {
#pragma unroll
        for (int i = 0; i < PA; ++i)
          if (a_piece(i)) glds16_buf(rs_a, a_off[i], koff, base + i * NT * 16);
      } else if (part == 1) {
        w_half(std::integral_constant<int, PA>{});
      } else if (part == 2) {
        w_half(std::integral_constant<int, PA + HW>{});
        koff += 128;
      }
      return;
    }
  };

  // Hand-placed schedules (SCHED 7 / 8): the tile's PA + PW requests are dealt to the first kParts K steps, PER per step, one
  // statement of up to four requests (A pieces that not every wave owns go singly behind their wave-uniform test).
  constexpr int kParts = kFillParts;
  constexpr int PER = (PA + PW + kParts - 1) / kParts;
  static_assert(!kM16 || ADDR >= 1, "hand-placed schedules use the buffer-form LDS-DMA");
  auto fill_batched = [&](int buf, auto part_c) __attribute__((always_inline)) {
    constexpr int part = decltype(part_c)::value;
    constexpr int P0 = part * PER, P1 = (P0 + PER < PA + PW) ? P0 + PER : PA + PW;
    if constexpr (ADDR >= 1 && P0 < P1) {
      const unsigned base = lds0 + buf * STAGE + wave * 1024;
      constexpr int G0 = PA_MIN, G1 = PA;   // [G0, G1): A pieces only the first waves own
#pragma unroll
      for (int idx = (P0 > G0 ? P0 : G0); idx < (P1 < G1 ? P1 : G1); ++idx)
        if (a_piece(idx)) glds16_buf(rs_a, a_off[idx < PA ? idx : 0], koff, base + idx * NT * 16);
      constexpr int NU = count_outside(P0, P1, G0, G1);
      auto batch = [&](auto b_c) {
        constexpr int b = decltype(b_c)::value;
        constexpr int n = NU - 4 * b >= 4 ? 4 : NU - 4 * b;
        if constexpr (n > 0) {
          constexpr int I0 = nth_outside(P0, P1, G0, G1, 4 * b), I1 = n > 1 ? nth_outside(P0, P1, G0, G1, 4 * b + 1) : I0,
                        I2 = n > 2 ? nth_outside(P0, P1, G0, G1, 4 * b + 2) : I0, I3 = n > 3 ? nth_outside(P0, P1, G0, G1, 4 * b + 3) : I0;
          glds16_buf_n<n, piece_lds(I0), piece_lds(I1), piece_lds(I2), piece_lds(I3)>(
              base, koff, piece_rs(I0), piece_vo(I0), piece_rs(I1), piece_vo(I1), piece_rs(I2), piece_vo(I2), piece_rs(I3), piece_vo(I3));
        }
      };
      static_assert(NU <= 12, "three batches of four per K step");
      batch(std::integral_constant<int, 0>{});
      batch(std::integral_constant<int, 1>{});
      batch(std::integral_constant<int, 2>{});
      if constexpr (P1 == PA + PW) koff += 128;
    }
  };
  auto fill_part_placed = [&](int buf, int part) __attribute__((always_inline)) {
    if (part == 0) fill_batched(buf, std::integral_constant<int, 0>{});
    else if (part == 1) fill_batched(buf, std::integral_constant<int, 1>{});
    else if (part == 2) fill_batched(buf, std::integral_constant<int, 2>{});
  };

  // ---- ADDR 2: the A tile gathered from fp32 pixels (im2col on load) ------------------------------------------------
  // A K tile of 64 columns = 64 / P patch rows u of one channel c (P = 32: two rows, P = 16: four), 64 consecutive k = (c, u, v).
  // Thread -> load q = pass * NT + tid: tile row q >> 4, four-pixel group q & 15 of the row's 64 columns.  The per-lane byte offset
  // into the pixels never changes inside the K loop; the tile's (c, u0) is a wave-uniform scalar offset.  Two register sets: the
  // loads of tile kt+2 travel while tile kt+1's values are converted and written to its LDS stage (K loop unrolled by two, so
  // the sets are compile-time).
  i32x4 rs_p;
  unsigned pix_off[kGather ? NAL : 1];
  int ga_dst[kGather ? NAL : 1];
  using GA = std::conditional_t<kGatherU8, u32x3, u32x4>;
  GA ga[2][kGather ? NAL : 1];
  if constexpr (kGather) {
    rs_p = kGatherU8 ? make_buffer_rsrc(p.tiles) : make_buffer_rsrc(p.pix);
    const int P = 1 << p.patch_log2, gw = p.img_w >> p.patch_log2, f4_per_row = P >> 2;   // patch side, patches per image row
#pragma unroll
    for (int i = 0; i < NAL; ++i) {
      const int q = i * NT + tid, row = q >> 4, f4 = q & 15;
      int r = m0 + row;
      r = r < Mrt ? r : Mrt - 1;
      const int img = r / p.np, pp = r - img * p.np, gi = pp / gw, gj = pp - gi * gw;
      const int j = f4 / f4_per_row, gq = f4 - j * f4_per_row;        // patch row inside the K tile, four-pixel group inside it
      if constexpr (kGatherU8)   // HWC bytes: pixel (img, y, x) at ((img * H + y) * W + x) * 3; the channel is picked after the load
        pix_off[i] = (unsigned)((((size_t)img * p.img_h + gi * P + j) * p.img_w + gj * P + gq * 4) * 3);
      else                       // NCHW fp32: pixel (img, c, y, x) at ((img * 3 + c) * H + y) * W + x; the channel is in the scalar offset
        pix_off[i] = (unsigned)((((size_t)img * 3 * p.img_h + gi * P + j) * p.img_w + gj * P + gq * 4) * 4);
      const int kl = j * P + gq * 4;                                   // column inside the K tile: 16-byte chunk kl >> 3, half (kl >> 2) & 1
      ga_dst[i] = row * 128 + ((((kl >> 3) ^ ((row >> 1) & 7))) << 4) + ((kl >> 2) & 1) * 8;
    }
  }
  // scalar byte offset of K tile t inside an image: channel c = t / (P * P / 64), first patch row u0 = (t % (P * P / 64)) * (64 / P)
  auto gather_soff = [&](int t) __attribute__((always_inline)) -> unsigned {
    const int tpc_log2 = 2 * p.patch_log2 - 6;
    const int c = t >> tpc_log2, u0 = (t & ((1 << tpc_log2) - 1)) << (6 - p.patch_log2);
    if constexpr (kGatherU8) return (unsigned)(u0 * p.img_w * 3);
    return (unsigned)((c * p.img_h + u0) * p.img_w * 4);
  };
  constexpr int NALX = kGather ? NAL : 1;
  auto gather_load = [&](GA (&set)[NALX], int t) __attribute__((always_inline)) {
    if constexpr (kGather) {
      const unsigned soff = gather_soff(t);
#pragma unroll
      for (int i = 0; i < NAL; ++i) {
        if constexpr (kGatherU8) pix_load12(set[i], pix_off[i], rs_p, soff);
        else pix_load16(set[i], pix_off[i], rs_p, soff);
      }
    }
  };
  // (leave: how many of this wave's vector-memory requests may still be outstanding -- one tile's, or none)
  auto gather_wait = [&](GA (&set)[NALX], bool one_tile) __attribute__((always_inline)) {
    if constexpr (kGather) {
      static_assert(NAL == 5, "the wait statement names five register sets");
      if (one_tile) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NAL + PW) : "memory");
      else wait_vm0();
      tie_regs5(set[0], set[1], set[2], set[3], set[4]);
    }
  };
  // t: the K tile the set holds (uint8 tiles: its channel picks the bytes and the normalisation constants; wave-uniform)
  auto gather_store = [&](GA (&set)[NALX], int stage, int t) __attribute__((always_inline)) {   // -> operand type (the unfold kernels' rounding), into the A stage
    if constexpr (kGather && sizeof(T) == 2) {
      using Th = std::conditional_t<sizeof(T) == 2, T, bf16_t>;
      using X4h = typename half_traits<Th>::x4;
      if constexpr (kGatherU8) {
        const int c = t >> (2 * p.patch_log2 - 6);
        auto put = [&](auto c_c) __attribute__((always_inline)) {
          constexpr int C = decltype(c_c)::value;        // the lane's four pixels are bytes C, C + 3, C + 6, C + 9 of its twelve
#pragma unroll
          for (int i = 0; i < NAL; ++i) {
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int byte = C + 3 * e;
              v[e] = u8_norm((float)((set[i][byte >> 2] >> (8 * (byte & 3))) & 0xffu), C);
            }
            const X4h pk = {from_f32<Th>(v[0]), from_f32<Th>(v[1]), from_f32<Th>(v[2]), from_f32<Th>(v[3])};
            *reinterpret_cast<X4h*>(smem + stage * STAGE + ga_dst[i]) = pk;
          }
        };
        if (c == 0) put(std::integral_constant<int, 0>{});
        else if (c == 1) put(std::integral_constant<int, 1>{});
        else put(std::integral_constant<int, 2>{});
      } else {
#pragma unroll
        for (int i = 0; i < NAL; ++i) {
          const f32x4 v = __builtin_bit_cast(f32x4, set[i]);
          const X4h pk = {from_f32<Th>(v[0]), from_f32<Th>(v[1]), from_f32<Th>(v[2]), from_f32<Th>(v[3])};
          *reinterpret_cast<X4h*>(smem + stage * STAGE + ga_dst[i]) = pk;
        }
      }
    }
  };

  // ---- fragment read offsets (lane-constant) -----------------------------------
  const int lrow = lane & 31, lgrp = lane >> 5;
  const int lsw = (lrow >> 1) & 7;
  int foff[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) foff[ks] = lrow * 128 + (((ks * 2 + lgrp) ^ lsw) << 4);
  const int a_tile = wm * TM * 128;
  const int w_tile = A_BYTES + wn * TN * 128;

  struct Unused {};   // the type of a form's state in the instantiations of the other forms: every use sits behind `if constexpr`
  // (16x16x32 forms: a one-block dummy that nothing reads.  Taking it out -- the other form's name as an empty struct, as for acc4 below --
  //  changes the instruction order of the ring tile's EPI_SCALE kernel, 1044 -> 1043 instructions, and of no other: it stays until a
  //  change that alters the kernels anyway; profiles/gemm_split_isa.txt)
  f32x16 acc[kM16 ? 1 : MI][kM16 ? 1 : NI];
#pragma unroll
  for (int i = 0; i < (kM16 ? 1 : MI); ++i)
#pragma unroll
    for (int j = 0; j < (kM16 ? 1 : NI); ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  // 16x16x32 form: the wave's 32x32 blocks as four 16x16 tiles each.  acc4[2i+b][2j+a][e] = C[m = 32i + 16b + (lane & 15)]
  // [n = 32j + 16a + 4 (lane >> 4) + e]: a lane holds TWO rows of a block (b = 0, 1) and, per row, 4 consecutive columns in each
  // 16-column half -- again whole 16-byte fp32 / 8-byte 16-bit pieces of an output row.
  // rows of a wave row's 32-row slab i that exist (kHalf: the last slab may be a half slab)
  auto slab_rows = [](int i) constexpr { return kHalf ? (TM - 32 * i < 32 ? TM - 32 * i : 32) : 32; };
  std::conditional_t<kM16, f32x4[MI2][NI2], Unused> acc4;
  if constexpr (kM16) {
#pragma unroll
    for (int i = 0; i < MI2; ++i)
#pragma unroll
      for (int j = 0; j < NI2; ++j) acc4[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const int l16 = lane & 15, g16 = lane >> 4;

  // epilogue operands in the row-contiguous layout of the transposed store (16 lanes x 16 B per output row)
  // Register budget (256 per lane at two waves per SIMD): accumulators + K-loop fragments + one operand block must
  // fit for the early request, accumulators + two operand blocks + the transposed values for the double buffer;
  // the 192x256 / 160x256 tiles afford both, 320x256 and the 4x2-wave 256x256 tile neither (they would spill).
  const int rd_row = lane >> 4, rd_col = (lane & 15) * 4;
  float4 add[kAddBufs][NI / 2][8];
  bool add_ready = false;
  auto load_block = [&](int i, float4 (&dst)[NI / 2][8]) {
    if constexpr (EPI == EPI_RESID_SPLIT) {
      // the residual planes in 16-byte pieces: a lane owns 8 consecutive columns of a row (8 lanes = one 64-column slice), 8 rows per
      // pass.  dst[jp][it] = hi piece of pass it (8 x 16-bit operand type); dst[jp][4 + pr] = lo piece of the pass PAIR pr: the 8-bit
      // remainders of the lane's columns in rows r and r + 8 of a 16-row band (common.h lo_plane_off) -- 6 loads per slab, not 8
#pragma unroll
      for (int jp = 0; jp < NI / 2; ++jp) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
          if (it * 8 >= slab_rows(i)) continue;   // half slab: rows 16.. belong to the next wave row
          int m = m0 + wm * TM + i * 32 + it * 8 + (lane >> 3);
          m = m < Mrt ? m : Mrt - 1;
          const size_t off = (size_t)m * p.ldc + n0 + wn * TN + jp * 64 + (lane & 7) * 8;
          dst[jp][it] = *reinterpret_cast<const float4*>(reinterpret_cast<const unsigned short*>(p.xb_out) + off);
        }
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {
          if (pr * 16 >= slab_rows(i)) continue;
          int band = (m0 + wm * TM + i * 32 + pr * 16) >> 4;
          band = band < ((Mrt - 1) >> 4) ? band : ((Mrt - 1) >> 4);      // bands past the live rows: re-read the last one, stores are masked
          const size_t off = (size_t)band * 16 * p.ldc + (size_t)(((n0 + wn * TN + jp * 64) >> 3) + (lane & 7)) * 128 + (lane >> 3) * 16;
          dst[jp][4 + pr] = *reinterpret_cast<const float4*>(reinterpret_cast<const unsigned char*>(p.lo_io) + off);
        }
      }
    } else {
#pragma unroll
      for (int jp = 0; jp < NI / 2; ++jp)
#pragma unroll
        for (int it = 0; it < 8; ++it) {
          if (it * 4 >= slab_rows(i)) continue;
          const int m = m0 + wm * TM + i * 32 + it * 4 + rd_row;
          dst[jp][it] = EpilogueOp<T, EPI>::load(p, m < Mrt ? m : Mrt - 1, n0 + wn * TN + jp * 64 + rd_col);
        }
    }
  };

  // ---- hand-placed K step, 16x16x32 form (SCHED 7 / 8) ---------------------------------------------------------
  // A K tile is TWO steps of 32.  Per step the wave needs MI2 activation fragments (16 rows x 32 k: lane = row l16, 16-byte
  // chunk 4s + g16 of the 128-byte LDS row; the XOR swizzle keeps every ds_read_b128 lane group on 16 distinct slots) and NI2
  // weight fragments, and issues MI2 * NI2 MFMAs.
  //  * two LDS stages: the operand with FEWER fragments (always 4 here) is KEPT in registers for the step (double-buffered
  //    across steps), the other is STREAMED -- one fragment per group of 4 MFMAs (below).
  //  * ring of three (barrier IN FRONT of the tile's last step): behind that barrier nobody may read the tile's stage any more
  //    -- the next iteration's fill overwrites it -- so every fragment of a step is read during the step before it (both operands
  //    double-buffered whole), one read per MFMA slot, and the last step's slots carry the NEXT tile's first fragments.
  // A scheduling fence closes every slot.
  constexpr bool kStream16 = NSTAGE == 2;
  constexpr bool kKeepX = MI2 <= NI2;                 // (streamed form) keep the activation fragments, stream the weights -- or the reverse
  constexpr int NK = kKeepX ? MI2 : NI2, NS = kKeepX ? NI2 : MI2;
  static_assert(!kM16 || !kStream16 || (NK == 4 && NS >= 4), "streamed 16x16x32 form: four kept fragments, at least four streamed ones");
  static_assert(!kM16 || !kUneven, "the 16x16x32 forms deal wave rows in 16-row blocks: every wave row holds the same MI2 of them");
  int foff16[2];
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) foff16[s2] = l16 * 128 + (((4 * s2 + g16) ^ (l16 >> 1)) << 4);
  using H16 = std::conditional_t<sizeof(T) == 2, T, bf16_t>;
  using X8h = typename half_traits<H16>::x8;
  auto x_frag = [&](const char* sb, int s2, int ii) __attribute__((always_inline)) {
    return *reinterpret_cast<const u32x4*>(sb + a_tile + ii * 16 * 128 + foff16[s2]);
  };
  auto w_frag = [&](const char* sb, int s2, int jj) __attribute__((always_inline)) {
    return *reinterpret_cast<const u32x4*>(sb + w_tile + jj * 16 * 128 + foff16[s2]);
  };
  auto mma16x16 = [&](int ii, int jj, const u32x4& wf, const u32x4& xf) __attribute__((always_inline)) {
    if constexpr (kM16) acc4[ii][jj] = half_traits<H16>::mfma16(__builtin_bit_cast(X8h, wf), __builtin_bit_cast(X8h, xf), acc4[ii][jj]);
  };
  std::conditional_t<SCHED == 8, u32x4[2][4], Unused> kf16;   // SCHED 8 state: the kept fragments of both steps ...
  auto keep_frag = [&](const char* sb, int s2, int u) __attribute__((always_inline)) { return kKeepX ? x_frag(sb, s2, u) : w_frag(sb, s2, u); };
  auto stream_frag = [&](const char* sb, int s2, int t) __attribute__((always_inline)) { return kKeepX ? w_frag(sb, s2, t) : x_frag(sb, s2, t); };
  // ---- streamed form (SCHED 8).  The streamed fragments of a tile form ONE sequence g = step * NS + t over both steps, read two
  //      groups ahead (one group = 4 MFMAs = 64 pipe cycles, 128 with the SIMD's other wave in between: one group of lookahead
  //      does not cover an LDS round trip under load).  The tile's barrier sits IN FRONT of its last PB groups: every LDS read of
  //      a tile still lies between the tile's two barriers, but the last PB groups' stream fragments are read early (two fragments per group over the groups
  //      before them, then one group of slack for the LDS round trip), so behind the barrier 4 PB MFMAs run from registers while the
  //      NEXT tile's kept fragments and first two stream fragments arrive -- barrier wait and LDS round trip under matrix work.
  //      PB = 4 on both tiles (320x256, 160 accumulator registers: 3407 -> 3249 cycles per K tile against PB = 2; its plain epilogues
  //      spill 3-17 registers outside the loop either way, the LayerNorm-folded fc1 epilogue none).
  constexpr int G16 = 2 * NS;
  constexpr int PB16 = 4;
  constexpr int GD16 = G16 - 2 * PB16;                 // first group that reads two stream fragments
  std::conditional_t<SCHED == 8, u32x4[SCHED == 8 ? G16 : 1], Unused> sfr;   // ... and the tile's streamed fragments
  auto prime16 = [&](const char* sb) __attribute__((always_inline)) {
    if constexpr (SCHED == 8) {
      sfr[0] = stream_frag(sb, 0, 0);
#pragma unroll
      for (int u = 0; u < 4; ++u) kf16[0][u] = keep_frag(sb, 0, u);
      sfr[1] = stream_frag(sb, 0, 1);
    }
  };
  // groups [g0, g1) of the tile in stage sb; sbn: the next tile's stage for the groups behind the barrier (has_next)
  auto groups16 = [&](const char* sb, int g0, int g1, int fill_buf, int nparts, const char* sbn, bool has_next) __attribute__((always_inline)) {
    if constexpr (SCHED == 8)
#pragma unroll
    for (int g = 0; g < G16; ++g) {
      if (g < g0 || g >= g1) continue;
      const int s2 = g / NS, t = g % NS;
      const bool post = g >= G16 - PB16;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int us = (g & 1) ? 3 - u : u;             // serpentine over the kept fragments: one operand changes per MFMA
        if (kKeepX) mma16x16(us, t, sfr[g], kf16[s2][us]);
        else mma16x16(t, us, kf16[s2][us], sfr[g]);
        if (!post) {
          if (g < GD16) {
            if (u == 0 && g + 2 < G16) sfr[g + 2] = stream_frag(sb, (g + 2) / NS, (g + 2) % NS);
          } else {
            const int f = GD16 + 2 + 2 * (g - GD16) + (u >> 1);
            if ((u == 0 || u == 2) && f < G16) sfr[f] = stream_frag(sb, f / NS, f % NS);
          }
          if (s2 == 0 && u == 1 && t < 4) kf16[1][t] = keep_frag(sb, 1, t);
          if (s2 == 0 && u == 3 && fill_buf >= 0 && t < nparts) fill_part_placed(fill_buf, t);
        } else if (has_next && u < 3) {
          const int r = (g - (G16 - PB16)) * 3 + u;     // 0: stream 0, 1..4: kept 0..3, 5: stream 1
          if (r == 0) sfr[0] = stream_frag(sbn, 0, 0);
          else if (r <= 4) kf16[0][r - 1] = keep_frag(sbn, 0, r - 1);
          else if (r == 5) sfr[1] = stream_frag(sbn, 0, 1);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  };
  // ---- fully double-buffered form (ring of three)
  std::conditional_t<SCHED == 7, u32x4[2][MI2], Unused> xf16;   // SCHED 7 state: both operands' fragments of two steps
  std::conditional_t<SCHED == 7, u32x4[2][NI2], Unused> wf16;
  constexpr int NR16 = MI2 + NI2;                      // fragment reads of a step, in the order below
  static_assert(!kM16 || kStream16 || NR16 <= MI2 * NI2, "ring form: one fragment read per MFMA slot");
  // read r of a step: the x fragments, then the w's
  auto read16 = [&](const char* sb, int s2, int b, int r) __attribute__((always_inline)) {
    if constexpr (SCHED == 7) {
      if (r < MI2) xf16[b][r] = x_frag(sb, s2, r);
      else wf16[b][r - MI2] = w_frag(sb, s2, r - MI2);
    }
  };
  auto read16_all = [&](const char* sb, int s2, int b) __attribute__((always_inline)) {
#pragma unroll
    for (int r = 0; r < NR16; ++r) read16(sb, s2, b, r);
  };
  // b: fragment buffer of this step; (sbn, sn): the step whose fragments are read meanwhile into b ^ 1 (sn < 0: none)
  auto step16_full = [&](int b, const char* sbn, int sn, int fill_buf, int nparts) __attribute__((always_inline)) {
    if constexpr (SCHED == 7)
#pragma unroll
    for (int ii = 0; ii < MI2; ++ii) {
#pragma unroll
      for (int jj = 0; jj < NI2; ++jj) {
        const int n = ii * NI2 + jj;
        const int js = (ii & 1) ? NI2 - 1 - jj : jj;   // serpentine: one operand changes per MFMA, also at a row change (+0.5-1.5 % warm)
        mma16x16(ii, js, wf16[b][js], xf16[b][ii]);
        if (sn >= 0 && n < NR16) read16(sbn, sn, b ^ 1, n);
        if (fill_buf >= 0 && jj == NI2 - 1 && ii >= 1 && ii - 1 < nparts) fill_part_placed(fill_buf, ii - 1);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  };

  // ---- 32x32 forms (SCHED 0 / 1 / 6): the fragments of one K step for the wave's MI x NI blocks, double-buffered; the fragments of
  // K-step ks+1 are fetched from LDS before the MFMAs of step ks issue.  (Rows past an uneven wave row's
  // last block are read too -- in-bounds LDS bytes nobody multiplies -- so the reads stay branch-free: skipping them behind a
  // wave-uniform branch measured 47.2 vs 44.6 us per launch of the residual GEMMs in the step.)
  std::conditional_t<kM16, Unused, u32x4[2][MI]> xf;
  std::conditional_t<kM16, Unused, u32x4[2][NI]> wf;
  auto read_frags = [&](const char* sb, int ks, int b) {
    if constexpr (!kM16) {
#pragma unroll
      for (int i = 0; i < MI; ++i) xf[b][i] = *reinterpret_cast<const u32x4*>(sb + a_tile + i * 32 * 128 + foff[ks]);
#pragma unroll
      for (int j = 0; j < NI; ++j) wf[b][j] = *reinterpret_cast<const u32x4*>(sb + w_tile + j * 32 * 128 + foff[ks]);
    }
  };
  auto mma_step = [&](int b) {
    if constexpr (!kM16) {
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        if (kUneven && i >= mi_w) break;   // wave-uniform
#pragma unroll
        for (int j = 0; j < NI; ++j) mma16<T>(acc[i][j], wf[b][j], xf[b][i]);
      }
    }
  };
  // one K tile on two stages; the next fill's parts ride in its first K steps (SCHED 6)
  auto compute = [&](int buf, int fill_buf) {
    const char* sb = smem + buf * STAGE;
    read_frags(sb, 0, 0);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      if (ks < 3) read_frags(sb, ks + 1, (ks + 1) & 1);
      if constexpr (kSpread) {
        if (fill_buf >= 0 && ks < kFillParts) stage_issue_part(fill_buf, ks);
      }
      if constexpr (SCHED >= 1) __builtin_amdgcn_sched_barrier(0);
      mma_step(ks & 1);
      if constexpr (SCHED >= 1) __builtin_amdgcn_sched_barrier(0);
    }
  };

  // rstd of this tile's BM LayerNorm-input rows goes to LDS once, while the first K tile is in flight: the epilogue
  // then reads one float per row instead of walking the partials (a chain of L2 round trips per row) before the stores.
  // (Round 6: requesting the partials BEFORE the first fill and folding them behind it -- so that the compiler's vmcnt for these loads
  //  does not drain the inline-asm fills first -- measured level on fc1 / q/k/v and on the step, and is not done.)
  auto stage_ln_rows = [&]() {
    if constexpr (epi_is_ln(EPI)) {
      float* ln_rows = reinterpret_cast<float*>(smem + NSTAGE * STAGE);
      for (int r = tid; r < BM; r += NT) {
        const int mr = m0 + r < Mrt ? m0 + r : Mrt - 1;
        float mu, rs;
        ln_combine(p.ln_stats + (size_t)mr * p.ln_ns * 2, p.ln_ns, p.ln_inv_d, p.ln_eps, mu, rs);
        ln_rows[r] = rs;
      }
    }
  };

  // ---- main loop: tiles kt+1 (and kt+2) stream in while tile kt is multiplied; one barrier per tile.
  const int KT = p.K / BK;
  unsigned long long* trace = p.trace ? p.trace + (size_t)bid * 8 : nullptr;
  unsigned long long trace_real0 = 0;
  if (trace && tid == 0) {
    trace[0] = __builtin_amdgcn_s_memtime();
    trace_real0 = __builtin_amdgcn_s_memrealtime();   // 100 MHz, one counter for the whole device (s_memtime is per XCD)
    trace[4] = lid;
    trace[5] = __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 4 /* HW_ID [31:0] */) |
               ((unsigned long long)__builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20 /* XCC_ID [3:0] */) << 32);
    trace[6] = (unsigned long long)KT |
               ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 6 /* LDS_ALLOC [31:0] */) << 32);
  }
  if constexpr (NSTAGE == 3) {
    // Ring of three.  Invariants at the top of iteration kt: tile kt is visible and its K-step-0 fragments are in registers;
    // tile kt+1 is landing or landed; the stage of tile kt-1 is free (every wave's reads of it had returned before the
    // barrier of iteration kt-1), so the fill of tile kt+2 goes there.  The wait in front of the barrier leaves one tile's
    // requests of this wave outstanding (vmcnt retires in order): tile kt+1 has landed, tile kt+2 may still fly.
    constexpr int kLeave = PA_MIN + PW;
    if constexpr (kGather) {
      // tile 0 -> set 0 / stage 0, tile 1 -> set 1 / stage 1; tile 0's pixels are rounded and written before the first barrier
      gather_load(ga[0], 0);
      stage_issue(0);
      if (KT > 1) { gather_load(ga[1], 1); stage_issue(1); }
      gather_wait(ga[0], KT > 1);
      gather_store(ga[0], 0, 0);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    } else {
      stage_issue(0);
      if (KT > 1) stage_issue(1);
      stage_ln_rows();
      if (KT > 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kLeave) : "memory");  // tile 0 landed, tile 1 may be in flight
      else wait_vm0();
    }
    __syncthreads();
    if (trace && tid == 0) trace[1] = __builtin_amdgcn_s_memtime();
    int cur = 0, nxt = 1, nxt2 = 2;  // stages of tiles kt, kt+1, kt+2
    if constexpr (kM16 && kGather) {
      using C0 = std::integral_constant<int, 0>; using C1 = std::integral_constant<int, 1>;
      // iteration kt (tile kt in stage cur, set S = kt & 1 free: tile kt's values were written to LDS an iteration ago)
      // (fetch_c = 0: the loop's odd last iteration, kt = KT - 2, has no tile kt + 2 -- said at compile time, so that no pixel load
      //  whose registers nobody reads afterwards is emitted there: hipcc gave five such dead loads ONE destination and reused it
      //  straight away, harmless only because the run-time test never took them; tests/test_isa_audit.py found it)
      auto iter = [&](auto s_c, auto fetch_c, int kt) __attribute__((always_inline)) {
        constexpr int S = decltype(s_c)::value;
        constexpr bool kMayFetch = decltype(fetch_c)::value != 0;
        const int fb = (kMayFetch && kt + 2 < KT) ? nxt2 : -1;
        if constexpr (kMayFetch) { if (fb >= 0) gather_load(ga[S], kt + 2); }
        const char* sc = smem + cur * STAGE;
        step16_full(0, sc, 1, fb, kParts);            // W pieces of tile kt+2 ride in this step
        // tile kt+1: its pixels (set S ^ 1) and this wave's W pieces have arrived -- only tile kt+2's requests may be outstanding;
        // round and write its A rows, publish, then the last step's MFMAs with the next tile's first fragment reads
        gather_wait(ga[S ^ 1], fb >= 0);
        gather_store(ga[S ^ 1], nxt, kt + 1);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __syncthreads();
        __builtin_amdgcn_sched_barrier(0);
        step16_full(1, smem + nxt * STAGE, 0, -1, 0);
        cur = nxt; nxt = nxt2; nxt2 = 3 - cur - nxt;
      };
      read16_all(smem, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      int kt = 0;
      for (; kt + 1 < KT - 1; kt += 2) { iter(C0{}, C1{}, kt); iter(C1{}, C1{}, kt + 1); }
      if (kt < KT - 1) iter(C0{}, C0{}, kt);
      if constexpr (kRowOperand) { load_block(0, add[0]); add_ready = true; __builtin_amdgcn_sched_barrier(0); }   // first epilogue block travels during the last K tile
      const char* sc = smem + cur * STAGE;
      step16_full(0, sc, 1, -1, 0);
      step16_full(1, sc, -1, -1, 0);
    } else if constexpr (kM16) {
      read16_all(smem, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      for (int kt = 0; kt < KT - 1; ++kt) {
        const int fb = kt + 2 < KT ? nxt2 : -1;
        const char* sc = smem + cur * STAGE;
        step16_full(0, sc, 1, fb, kParts);            // the whole fill of tile kt+2 rides in this step (the counted wait below)
        // this wave's pieces of tile kt+1 have landed and its last reads of tile kt have returned: publish, then the last step's
        // MFMAs (registers only) with the next tile's first fragment reads between them
        publish_tile<kLeave>(fb >= 0);
        __builtin_amdgcn_sched_barrier(0);
        step16_full(1, smem + nxt * STAGE, 0, -1, 0);
        cur = nxt; nxt = nxt2; nxt2 = 3 - cur - nxt;
      }
      if constexpr (kRowOperand) { load_block(0, add[0]); add_ready = true; __builtin_amdgcn_sched_barrier(0); }   // first epilogue block travels during the last K tile
      const char* sc = smem + cur * STAGE;
      step16_full(0, sc, 1, -1, 0);
      step16_full(1, sc, -1, -1, 0);
    } else {
      read_frags(smem, 0, 0);
      for (int kt = 0; kt < KT - 1; ++kt) {
        const bool fetch = kt + 2 < KT;
        if constexpr (!kSpread) { if (fetch) stage_issue(nxt2); }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          if (ks < 3) {
            read_frags(smem + cur * STAGE, ks + 1, (ks + 1) & 1);
            if constexpr (kSpread) { if (fetch && ks < kFillParts) stage_issue_part(nxt2, ks); }
          } else {
            // this wave's pieces of tile kt+1 have landed and its last reads of tile kt have returned: publish, then fetch
            // the next tile's first fragments while the MFMAs below run
            publish_tile<kLeave>(fetch);
            read_frags(smem + nxt * STAGE, 0, 0);
          }
          __builtin_amdgcn_sched_barrier(0);
          mma_step(ks & 1);
          __builtin_amdgcn_sched_barrier(0);
        }
        cur = nxt; nxt = nxt2; nxt2 = 3 - cur - nxt;   // rotate: the stage tile kt leaves becomes tile kt+3's
      }
      if constexpr (kRowOperand) { load_block(0, add[0]); add_ready = true; __builtin_amdgcn_sched_barrier(0); }   // first epilogue block travels during the last K tile
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        if (ks < 3) read_frags(smem + cur * STAGE, ks + 1, (ks + 1) & 1);
        __builtin_amdgcn_sched_barrier(0);
        mma_step(ks & 1);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  } else if constexpr (kM16) {
    // two stages, 16x16x32 form: the fill of tile kt+1 rides in the first groups of tile kt; one barrier per tile, in front of
    // the tile's last PB16 groups
    stage_issue(0);
    stage_ln_rows();
    wait_vm0();
    __syncthreads();
    if (trace && tid == 0) trace[1] = __builtin_amdgcn_s_memtime();
    prime16(smem);
    __builtin_amdgcn_sched_barrier(0);
    for (int kt = 0; kt < KT - 1; ++kt) {
      const char* sc = smem + (kt & 1) * STAGE;
      const char* sn = smem + ((kt & 1) ^ 1) * STAGE;
      groups16(sc, 0, G16 - PB16, (kt & 1) ^ 1, kParts, sn, false);
      publish_tile<0>(false);
      __builtin_amdgcn_sched_barrier(0);
      groups16(sc, G16 - PB16, G16, -1, 0, sn, true);
    }
    if constexpr (kRowOperand) { load_block(0, add[0]); add_ready = true; __builtin_amdgcn_sched_barrier(0); }   // first epilogue block travels during the last K tile
    groups16(smem + ((KT - 1) & 1) * STAGE, 0, G16, -1, 0, smem, false);
  } else {
    stage_issue(0);
    stage_ln_rows();
    wait_vm0();
    __syncthreads();
    if (trace && tid == 0) trace[1] = __builtin_amdgcn_s_memtime();
    for (int kt = 0; kt < KT - 1; ++kt) {
      const int cur = kt & 1;
      if constexpr (!kSpread) {
        stage_issue(cur ^ 1);
      }
      compute(cur, cur ^ 1);
      wait_vm0();
      __syncthreads();
    }
    if constexpr (kRowOperand) { load_block(0, add[0]); add_ready = true; __builtin_amdgcn_sched_barrier(0); }   // first epilogue block travels during the last K tile
    compute((KT - 1) & 1, -1);
  }
  if (trace && tid == 0) trace[2] = __builtin_amdgcn_s_memtime();

  // ---- epilogue -------------------------------------------------------------------------------
  // The accumulator layout gives a lane ONE output row: acc[i][j][4q+e] = C[m = .. + lrow][n = .. + 8q + 4*lgrp + e].
  // Stored straight from there every store instruction touches 32 different rows (64 scattered 16-byte
  // pieces), and the in-kernel timeline showed that costing 22-34k cycles per 256x256 tile -- a third of the
  // workgroup's lifetime.  So each wave transposes its sub-tile through a private LDS slab (32 rows x 64
  // columns fp32, row pitch 272 B: conflict-free ds_write_b128) and writes it back ROW-contiguous: 16 lanes
  // cover 256 B (fp32) / 128 B (16-bit) of one row, so loads/stores are whole cache lines.
  __syncthreads();  // every wave is done reading the last K tile: the staging LDS can be reused
  char* slab = smem + wave * SLAB_BYTES;
  if constexpr (sizeof(T) == 2 && epi_is_colwise(EPI)) {
    // 16-bit outputs whose epilogue is column-wise (bias, QuickGELU): finish the arithmetic in the ACCUMULATOR layout
    // -- the bias of a lane's 4 x 4 columns per MFMA tile is loaded once per tile column, not once per output row --
    // round there, and transpose HALF the bytes: 8 ds_write_b64 + 4 ds_read_b128 + 4 16-byte global stores
    // per 32 x 64 slab instead of 8 ds_write_b128 + 8 ds_read_b128 + 8 bias loads + 8 8-byte stores.
    // 16-bit slab: 32 rows x 128 B, no padding.  16-byte chunk c of row r sits in slot c ^ (r & 7) and, for rows with
    // bit 3 set, its two 8-byte halves are swapped: the transposing ds_write_b64 (16 consecutive rows, same column)
    // then covers all 32 write banks once, the row-contiguous ds_read_b128 all 64 read banks once
    // (SQ_LDS_BANK_CONFLICT = 0); the half swap is undone in registers, statically per store iteration.
    constexpr int HP = 128;
    using X4 = typename half_traits<OutT>::x4;
    // bias of this lane's columns: 32x32 form 4 columns at 8q + 4 lgrp of each 32-column block, 16x16 form at 16a + 4 g16
    float4 bq[NI][4];
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int q = 0; q < (kM16 ? 2 : 4); ++q)
        bq[j][q] = *reinterpret_cast<const float4*>(p.bias + n0 + wn * TN + j * 32 + (kM16 ? 16 * q + 4 * g16 : 8 * q + 4 * lgrp));
    const int hr_row = lane >> 3, hr_chunk = lane & 7;  // 8 lanes x 16 B = one 128-byte output row piece
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      if (kUneven && i >= mi_w) break;   // wave-uniform
      float ln_rs = 1.f, ln_rs2[2] = {1.f, 1.f};
      if constexpr (epi_is_ln(EPI)) {  // this lane's row(s) of the block: rstd of the LayerNorm input row (staged at kernel start)
        if constexpr (kM16) {
          ln_rs2[0] = *reinterpret_cast<const float*>(smem + NSTAGE * STAGE + (wm * TM + i * 32 + l16) * 4);
          if (slab_rows(i) > 16)
            ln_rs2[1] = *reinterpret_cast<const float*>(smem + NSTAGE * STAGE + (wm * TM + i * 32 + 16 + l16) * 4);
        } else {
          ln_rs = *reinterpret_cast<const float*>(smem + NSTAGE * STAGE + (wm * TM + i * 32 + lrow) * 4);
        }
      }
#pragma unroll
      for (int jp = 0; jp < NI / 2; ++jp) {
        if constexpr (kM16) {
          // 16x16 tiles (b = row half, a = column half) of the 32 x 64 slab: row 16b + l16, columns jj*32 + 16a + 4 g16 .. +3 ->
          // 16-byte chunk jj*4 + 2a + (g16 >> 1), 8-byte half g16 & 1; same swizzle as below (the 16 lanes of a ds_write_b64
          // group are again 16 consecutive rows of one column)
#pragma unroll
          for (int jj = 0; jj < 2; ++jj)
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
              for (int b = 0; b < 2; ++b) {
                if (16 * b >= slab_rows(i)) continue;
                const int j = 2 * jp + jj;
                const f32x4 c = acc4[2 * i + b < MI2 ? 2 * i + b : 0][2 * j + a];
                const X4 pk = finish_colwise<OutT, EPI>(c[0], c[1], c[2], c[3], ln_rs2[b], bq[j][a]);
                const int row = 16 * b + l16, chunk = jj * 4 + 2 * a + (g16 >> 1), half = g16 & 1;
                *reinterpret_cast<X4*>(slab + row * HP + ((chunk ^ (row & 7)) << 4) + ((half ^ ((row >> 3) & 1)) << 3)) = pk;
              }
        } else {
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int j = 2 * jp + jj;
            const X4 pk = finish_colwise<OutT, EPI>(acc[i][j][4 * q + 0], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2],
                                                    acc[i][j][4 * q + 3], ln_rs, bq[j][q]);
            *reinterpret_cast<X4*>(slab + lrow * HP + (((jj * 4 + q) ^ (lrow & 7)) << 4) +
                                   ((lgrp ^ ((lrow >> 3) & 1)) << 3)) = pk;
          }
        }
        __builtin_amdgcn_wave_barrier();
        u32x4 o[4];
#pragma unroll
        for (int it = 0; it < 4; ++it) {
          if (it * 8 >= slab_rows(i)) continue;
          const u32x4 raw = *reinterpret_cast<const u32x4*>(slab + (it * 8 + hr_row) * HP + ((hr_chunk ^ hr_row) << 4));
          o[it] = (it & 1) ? u32x4{raw[2], raw[3], raw[0], raw[1]} : raw;  // rows 8..15, 24..31: halves were swapped
        }
#pragma unroll
        for (int it = 0; it < 4; ++it) {
          if (it * 8 >= slab_rows(i)) continue;
          int m = m0 + wm * TM + i * 32 + it * 8 + hr_row;
          const bool in_range = m < Mrt;
          if (in_range)
            store16(reinterpret_cast<OutT*>(p.C) + (size_t)m * p.ldc + n0 + wn * TN + jp * 64 + hr_chunk * 8, o[it]);
        }
        __builtin_amdgcn_wave_barrier();
      }
    }
  } else {
    // every bias / residual / position row a 32-row block needs is requested one block ahead (block 0 before the last
    // K step), so the memory latency of the residual stream (MALL/HBM) is covered by the previous block's transpose
    if (!add_ready) load_block(0, add[0]);
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      if (kUneven && i >= mi_w) break;   // wave-uniform
      if constexpr (kAddBufs == 2) {
        if (i + 1 < MI && !(kUneven && i + 1 >= mi_w)) load_block(i + 1, add[(i + 1) & 1]);
      } else {
        if (i > 0) load_block(i, add[0]);
      }
#pragma unroll
      for (int jp = 0; jp < NI / 2; ++jp) {
        if constexpr (kM16) {   // row 16b + l16, columns jj*32 + 16a + 4 g16 .. +3 (8 consecutive lanes = 8 rows x 16 B: all 32 banks once)
#pragma unroll
          for (int jj = 0; jj < 2; ++jj)
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
              for (int b = 0; b < 2; ++b) {
                if (16 * b >= slab_rows(i)) continue;
                *reinterpret_cast<f32x4*>(slab + (16 * b + l16) * SLAB_PITCH + (jj * 32 + 16 * a + 4 * g16) * 4) =
                    acc4[2 * i + b < MI2 ? 2 * i + b : 0][2 * (2 * jp + jj) + a];
              }
        } else {
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const f32x4 v = {acc[i][2 * jp + jj][4 * q + 0], acc[i][2 * jp + jj][4 * q + 1], acc[i][2 * jp + jj][4 * q + 2],
                             acc[i][2 * jp + jj][4 * q + 3]};
            *reinterpret_cast<f32x4*>(slab + lrow * SLAB_PITCH + (jj * 32 + 8 * q + 4 * lgrp) * 4) = v;
          }
        }
        __builtin_amdgcn_wave_barrier();  // LDS ops of one wave execute in order; keep the compiler from reordering
        if constexpr (EPI == EPI_RESID_SPLIT) {
          // ---- split-plane epilogue.  8 columns per lane, 8 rows per pass: every global access of the two planes is a full 16-byte piece
          const int r8 = lane >> 3, c8 = (lane & 7) * 8;
          const int nn = n0 + wn * TN + jp * 64 + c8;
          const float4 b0 = *reinterpret_cast<const float4*>(p.bias + nn), b1 = *reinterpret_cast<const float4*>(p.bias + nn + 4);
          f32x4 va[4], vb[4];
#pragma unroll
          for (int it = 0; it < 4; ++it) {
            if (it * 8 >= slab_rows(i)) continue;
            va[it] = *reinterpret_cast<const f32x4*>(slab + (it * 8 + r8) * SLAB_PITCH + c8 * 4);
            vb[it] = *reinterpret_cast<const f32x4*>(slab + (it * 8 + r8) * SLAB_PITCH + c8 * 4 + 16);
          }
#pragma unroll
          for (int pr = 0; pr < 2; ++pr) {           // pass pairs: rows r8 and r8 + 8 of a 16-row band share one lo piece
            if (pr * 16 >= slab_rows(i)) continue;
            const u32x4 l = __builtin_bit_cast(u32x4, add[kAddBufs == 2 ? (i & 1) : 0][jp][4 + pr]);
            u32x4 lo4;
            const int m_first = m0 + wm * TM + i * 32 + pr * 16 + r8;
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
              const int it = 2 * pr + hh;
              const int m = m_first + 8 * hh;
              const bool in_range = m < Mrt;
              const u32x4 h = __builtin_bit_cast(u32x4, add[kAddBufs == 2 ? (i & 1) : 0][jp][it]);
              float o[8];
#pragma unroll
              for (int e = 0; e < 4; ++e) {             // columns 2e, 2e + 1: bytes 2e, 2e + 1 of this row's 8-byte half of the lo piece
                o[2 * e] = join_f32<T>(h[e] & 0xffffu, sbyte(l[2 * hh + (e >> 1)], (2 * e) & 3));
                o[2 * e + 1] = join_f32<T>(h[e] >> 16, sbyte(l[2 * hh + (e >> 1)], (2 * e + 1) & 3));
              }
              // (residual + bias) + product: the order of the plain-array epilogues
              o[0] = (o[0] + b0.x) + va[it][0]; o[1] = (o[1] + b0.y) + va[it][1]; o[2] = (o[2] + b0.z) + va[it][2];
              o[3] = (o[3] + b0.w) + va[it][3]; o[4] = (o[4] + b1.x) + vb[it][0]; o[5] = (o[5] + b1.y) + vb[it][1];
              o[6] = (o[6] + b1.z) + vb[it][2]; o[7] = (o[7] + b1.w) + vb[it][3];
              const float ssum = row8_sum(((o[0] + o[1]) + (o[2] + o[3])) + ((o[4] + o[5]) + (o[6] + o[7])));
              const float mj = ssum * (1.0f / kLnSlice);
              float q2 = 0.f;
#pragma unroll
              for (int e = 0; e < 8; ++e) { const float d = o[e] - mj; q2 = fmaf(d, d, q2); }
              const float m2 = row8_sum(q2);
              u32x4 ho;
              unsigned lb[8];
              using TO = std::conditional_t<std::is_same_v<T, bf16_t>, f16_t, bf16_t>;   // the other 16-bit type
              if (p.planes_other) {   // wave-uniform
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                  unsigned ha, hb;
                  split_f32<TO>(o[2 * e], ha, lb[2 * e]);
                  split_f32<TO>(o[2 * e + 1], hb, lb[2 * e + 1]);
                  ho[e] = ha | (hb << 16);
                }
              } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                  unsigned ha, hb;
                  split_f32<T>(o[2 * e], ha, lb[2 * e]);
                  split_f32<T>(o[2 * e + 1], hb, lb[2 * e + 1]);
                  ho[e] = ha | (hb << 16);
                }
              }
              lo4[2 * hh] = lb[0] | (lb[1] << 8) | (lb[2] << 16) | (lb[3] << 24);
              lo4[2 * hh + 1] = lb[4] | (lb[5] << 8) | (lb[6] << 16) | (lb[7] << 24);
              if (in_range) {
                store16(reinterpret_cast<unsigned short*>(p.xb_out) + (size_t)m * p.ldc + nn, ho);
                if ((lane & 7) == 0)
                  *reinterpret_cast<float2*>(p.st_out + ((size_t)m * (p.N / kLnSlice) + (n0 + wn * TN + jp * 64) / kLnSlice) * 2) =
                      make_float2(ssum, m2);
              }
            }
            // (a band's second row may lie past the live rows while its first does not: only the first row's 8-byte half is stored then --
            //  with a device-side row count the row behind it is a real row of the plane, not padding, and is not this call's to write)
            unsigned char* lo_dst = reinterpret_cast<unsigned char*>(p.lo_io) + (size_t)(m_first >> 4) * 16 * p.ldc + (size_t)((nn >> 3)) * 128 + r8 * 16;
            if (m_first + 8 < Mrt) store16(lo_dst, lo4);
            else if (m_first < Mrt) *reinterpret_cast<u32x2*>(lo_dst) = u32x2{lo4[0], lo4[1]};
          }
        } else {
          const int n = n0 + wn * TN + jp * 64 + rd_col;
          f32x4 v[8];
#pragma unroll
          for (int it = 0; it < 8; ++it) {
            if (it * 4 >= slab_rows(i)) continue;
            v[it] = *reinterpret_cast<const f32x4*>(slab + (it * 4 + rd_row) * SLAB_PITCH + rd_col * 4);
          }
#pragma unroll
          for (int it = 0; it < 8; ++it) {
            if (it * 4 >= slab_rows(i)) continue;
            int m = m0 + wm * TM + i * 32 + it * 4 + rd_row;
            const bool in_range = m < Mrt;
            if constexpr (EPI == EPI_RESID_EMIT) {
              // the updated residual row piece (4 columns per lane, 16 lanes = one 64-column slice of one row): fp32 in
              // place, its 16-bit copy for the next GEMM's A operand, and the slice's LayerNorm partials {sum, centred M2}
              const float4 a4 = add[kAddBufs == 2 ? (i & 1) : 0][jp][it];
              const float o0 = a4.x + v[it][0], o1 = a4.y + v[it][1], o2 = a4.z + v[it][2], o3 = a4.w + v[it][3];
              const float ssum = row16_sum((o0 + o1) + (o2 + o3));
              const float mj = ssum * (1.0f / kLnSlice);
              const float d0 = o0 - mj, d1 = o1 - mj, d2 = o2 - mj, d3 = o3 - mj;
              const float m2 = row16_sum((d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3));
              if (in_range) {
                store4(reinterpret_cast<float*>(p.C) + (size_t)m * p.ldc + n, o0, o1, o2, o3);
                store4(reinterpret_cast<OutT*>(p.xb_out) + (size_t)m * p.ldc + n, o0, o1, o2, o3);
                if ((lane & 15) == 0)
                  *reinterpret_cast<float2*>(p.st_out + ((size_t)m * (p.N / kLnSlice) + (n0 + wn * TN + jp * 64) / kLnSlice) * 2) =
                      make_float2(ssum, m2);
              }
            } else {
              if (in_range) EpilogueOp<T, EPI>::store(p, m, n, v[it][0], v[it][1], v[it][2], v[it][3], add[kAddBufs == 2 ? (i & 1) : 0][jp][it]);
            }
          }
        }
        __builtin_amdgcn_wave_barrier();
      }
    }
  }
  if (trace) {
    __builtin_amdgcn_s_waitcnt(0);  // stores issued and acknowledged before the stamp
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (tid == 0) {
      trace[3] = __builtin_amdgcn_s_memtime();
      trace[7] = (trace_real0 & 0xffffffffull) | ((__builtin_amdgcn_s_memrealtime() - trace_real0) << 32);
    }
  }
}

// One thread per output element; the on-device checker for the MFMA kernels
// (tests: variant -2), never used on the product path.
template <typename T, int EPI>
__global__ void gemm_nt_naive_kernel(const GemmParams p) {
  const int n4 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const int m = blockIdx.y;
  if (n4 >= p.N || m >= p.M) return;
  const T* a = reinterpret_cast<const T*>(p.A) + (size_t)m * p.lda;
  float v[4];
  for (int e = 0; e < 4; ++e) {
    const T* w = reinterpret_cast<const T*>(p.W) + (size_t)(n4 + e) * p.ldw;
    float s = 0.f;
    for (int k = 0; k < p.K; ++k) s = fmaf(to_f32(a[k]), to_f32(w[k]), s);
    v[e] = s;
  }
  EpilogueOp<T, EPI>::store(p, m, n4, v[0], v[1], v[2], v[3], EpilogueOp<T, EPI>::load(p, m, n4));
}

}  // namespace plipmi
