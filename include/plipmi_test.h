/*
 * plipmi_test.h -- kernel-level test entries and A/B hooks of libplipmi.so.
 *
 * NOT part of the product interface (include/plipmi.h, the drop-in boundary INTEGRATION.md maps to the reference's call
 * sites): these exports exist so that tests/ can compare single kernels with fp64 references through the same C ABI, and so
 * that tools/ can A/B tile choices on one box.  The product path (plip_amd/, bench.py's timed region) never calls them.
 * The plipmi_test_* setters are PROCESS-WIDE state (every handle, every later launch): test hooks only.
 */
#ifndef PLIPMI_TEST_H
#define PLIPMI_TEST_H

#include "plipmi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Parity tests only: run `tower` on `input` (pixels or ids; mask = NULL) through its
 * first `layer` blocks and copy the fp32 residual stream [B,S,D] to `out`
 * (layer 0 = embeddings, after pre_layrnorm for the vision tower -- HF hidden_states[layer]). */
int plipmi_debug_hidden(plipmi_handle h, int tower, int layer, const void* input, int B, float* out, void* stream);

/* Kernel-level entry for unit tests and micro-benchmarks of the GEMM that carries
 * >98 % of the path's FLOPs:  C = epilogue(A[M,K] * W[N,K]^T).
 *   dtype    PLIPMI_F32 | PLIPMI_BF16 | PLIPMI_F16 (A, W and non-fp32 outputs are that type; 16-bit types as raw uint16)
 *   epilogue 0: C(dtype) = acc + bias        1: C(dtype) = quickgelu(acc + bias)
 *            2: C(f32) += acc + bias         3: C(f32)   = alpha * acc
 *   variant  -1 = the engine's own choice, >= 0 = a specific tile configuration
 *            (plipmi_gemm_variant_name lists them; NULL past the end);
 *            variant -2 = the naive one-thread-per-output checker kernel;
 *            variant -3 = the small-M split-K kernel (16-bit types; epilogues 0..2; N % 64 == 0, K % 256 == 0). */
int plipmi_gemm_nt(int dtype, int epilogue, int variant, int M, int N, int K, const void* A, const void* W,
                   const float* bias, float alpha, void* C, void* stream);
const char* plipmi_gemm_variant_name(int variant);
/* 1 if this build of the library carries `variant` for `dtype`, else 0 */
int plipmi_gemm_variant_built(int dtype, int variant);
/* TEST / A-B HOOKS, process-wide, never called by the product path (the library reads no environment variables either).  Each
 * returns PLIPMI_OK, or PLIPMI_ERR_INVALID for a value outside its range (nothing changes then).  A hook changes what LATER launches
 * are; hipGraphs a handle captured earlier are dropped and re-captured at its next small-batch call.
 *   plipmi_test_force_gemm_tile(v)     every GEMM on tile v (0 .. n-1, plipmi_gemm_variant_name), -2 the naive checker kernel,
 *                                      -1 the engine's own cost model again
 *   plipmi_test_remap_gemm_tile(a, b)  where the cost model chooses tile a, run tile b (A/B runs of the whole step); b = -1 clears
 *   plipmi_test_fused_qkv_attention(m) the text tower's q/k/v projection + attention: 0 two kernels, 1 the product rule (fused where it
 *                                      applies and the batch fills the chip; default), 2 fused wherever it applies
 *   plipmi_test_patch_gather(on)       fp32 pixels: 0 unfold pass + plain patch GEMM, 1 im2col on load where it applies (default)
 *   plipmi_test_reset_hooks()          all of the above back to the product behaviour */
int plipmi_test_force_gemm_tile(int variant);
int plipmi_test_remap_gemm_tile(int from, int to);
int plipmi_test_fused_qkv_attention(int mode);
int plipmi_test_patch_gather(int on);
void plipmi_test_reset_hooks(void);
/* Test hook: the residual-stream planes {hi [rows, D] uint16, lo = the 8-bit remainder plane in its blocked layout,
 * ((rows + 15) / 16) * 16 * D bytes (plip_amd/csrc/common.h lo_plane_off)} from `from_dtype`'s split format to `to_dtype`'s
 * (PLIPMI_BF16 / PLIPMI_F16), in place -- what a text tower with plipmi_config.text_f16_layers does between its f16 and its
 * bf16 blocks on the small-M path.  The value is joined and split again: the new hi is the value rounded to the new operand type,
 * the remainder is rounded once more (2^-16 relative for bf16, 2^-19 for f16).  D % 8 == 0. */
int plipmi_recode_planes(void* hi, void* lo, size_t rows, int D, int from_dtype, int to_dtype, void* stream);
/* same call with explicit leading dimensions (in elements) for A [M,K] and W [N,K]: rows may be padded */
int plipmi_gemm_nt_ld(int dtype, int epilogue, int variant, int M, int N, int K, const void* A, int lda, const void* W,
                      int ldw, const float* bias, float alpha, void* C, void* stream);
/* same call with an in-kernel timeline: trace = device buffer of 8 x uint64 per workgroup
 * {start, prologue done, main loop done, epilogue done (s_memtime ticks: shader cycles, one counter per XCD), tile id,
 *  HW_ID|XCC_ID<<32, k tiles, start (low 32 bits) | lifetime << 32 in s_memrealtime ticks (100 MHz, device-wide)} */
int plipmi_gemm_nt_traced(int dtype, int epilogue, int variant, int M, int N, int K, const void* A, const void* W,
                          const float* bias, float alpha, void* C, uint64_t* trace, void* stream);

/* Kernel-level entry for the LayerNorm-folded epilogues of the 16-bit engines (gemm.h EPI_BIAS_LN / EPI_QGELU_LN /
 * EPI_RESID_EMIT / EPI_RESID_SPLIT; dtype PLIPMI_BF16 | PLIPMI_F16, A, W as raw uint16; "h16" below = that type):
 *   mode 0: C(h16) = rstd[m] * A.W^T + bias[n]       rstd from `stats` [M, ns, 2] fp32 = per-64-column partials (ns even)
 *   mode 1: C(h16) = quickgelu(that)                 {sum, centred M2} of the LayerNorm input rows (D = 64 * ns), eps as
 *                                                     given; W is expected to carry LayerNorm's gain with CENTRED rows
 *                                                     (sum_k W[n,k] = 0), which is what subtracts the row mean
 *   mode 2: C(f32) += A.W^T + bias;  xb_out(h16)[M,N] = C;  st_out [M, N/64, 2] = partials of the updated rows
 *   mode 3: the same update on a residual kept as two planes, xb_out = hi (uint16 [M, N]: the value rounded to h16) and
 *           C = lo (8-bit remainders in the blocked layout of plip_amd/csrc/common.h lo_plane_off, ((M + 15) / 16) * 16 * N bytes;
 *           bf16: bits(x) ~ (hi << 16) + (lo << 8), f16: x ~ hi + lo * 2^(E(hi) - 18)): the stream at 16 / 19 significand bits,
 *           both planes read and written in place; st_out as in mode 2.  This is the form the engine runs (6 bytes per element
 *           of epilogue traffic; the hi plane is the next GEMM's A operand)
 *   mode 4: mode 3 that READS the planes in dtype's split format and WRITES them in the other 16-bit type's (the last f16
 *           block of a bf16 text tower with plipmi_config.text_f16_layers hands the stream over without a re-coding pass)
 * variant as plipmi_gemm_nt; -3 (the small-M split-K kernel, K % 256 == 0) runs modes 0 .. 3 -- mode 3 there adds (x + bias) + A.W^T
 * as the tiles do, mode 2 x + (A.W^T + bias) -- and refuses mode 4: it writes the planes in the type it reads them in, the engine
 * re-codes them in a pass of their own on that path. */
int plipmi_gemm_nt_ln(int dtype, int mode, int variant, int M, int N, int K, const void* A, const void* W, const float* bias,
                      const float* stats, int ns, float eps, void* C, void* xb_out, float* st_out, void* stream);

/* Kernel-level entry for the exact-GELU epilogues (gemm.h EPI_BIAS_GELU / EPI_GELU_LN; the fc1 GEMM of a hidden_act = "gelu" tower):
 *   ln 0: C(T)   = gelu(A.W^T + bias[n])             every dtype; variant as plipmi_gemm_nt (-1, a tile, -2 the naive checker, and
 *                                                     -3 the small-M split-K kernel for the 16-bit types, K % 256 == 0)
 *   ln 1: C(h16) = gelu(rstd[m] * A.W^T + bias[n])   16-bit types only, stats / ns / eps as mode 1 of plipmi_gemm_nt_ln; variants -1,
 *                                                     a tile, -3 (the naive checker has no LayerNorm-folded form)
 * gelu(y) = 0.5 y (1 + erf(y / sqrt 2)); stats may be NULL and ns 0 for ln 0. */
int plipmi_gemm_nt_gelu(int dtype, int ln, int variant, int M, int N, int K, const void* A, const void* W, const float* bias,
                        const float* stats, int ns, float eps, void* C, void* stream);

/* Kernel-level entry for the text tower's fused kernel (csrc/qkv_attention.hip): LayerNorm-folded q/k/v projection (mode 0 of
 * plipmi_gemm_nt_ln with N = 3 * 64 H) with the attention in its epilogue, out [B*S, 64 H] -- bit-identical to
 * plipmi_gemm_nt_ln(mode 0) followed by plipmi_attention(impl 1).  dtype PLIPMI_BF16 | PLIPMI_F16, 65 <= S <= 80, ns = H.
 * (plipmi_test_fused_qkv_attention(0) makes the ENGINE run the two kernels instead, 1 the product rule, 2 the fused one at every batch.) */
int plipmi_qkv_attention(int dtype, const void* A, const void* W, const float* c2, const float* stats, int ns, float eps, void* out,
                         int B, int S, int H, int causal, const int64_t* key_mask,
                         uint64_t* trace /* NULL, or 8 x uint64 per workgroup: {start, prologue done, K loop done, Q/K/V images
                                            written, end (s_memtime), tile id, 0, start | lifetime << 32 (s_memrealtime)} */,
                         void* stream);

/* Kernel-level entry for the attention kernels: out[B*S, H*64] = softmax(q k^T + masks) v over the fused
 * activation qkv [B*S, 3*H*64] (q | k | v, 1/sqrt(64) already folded into q).
 *   impl 0 = exact-fp32 VALU kernel (any dtype), impl 1 = MFMA kernels (bf16 / f16; single pass for S <= 128, chunked
 *   online softmax beyond). */
int plipmi_attention(int dtype, int impl, const void* qkv, void* out, int B, int S, int H, int causal,
                     const int64_t* key_mask, void* stream);

/* The position-table resampler of plipmi_clone_resolution on its own: src fp32 [1 + n0*n0, D] (CLS row first) -> dst fp32
 * [1 + gh*gw, D]: the CLS row copied, the patch rows resampled as torch.nn.functional.interpolate(mode="bicubic",
 * align_corners=False) in fp32.  src and dst are distinct device buffers. */
int plipmi_resample_pos(const float* src, float* dst, int n0, int gh, int gw, int D, void* stream);

/* One evaluation of the linear-probe objective (csrc/probe.hip; arguments as plipmi_probe_fit in plipmi.h) at WB [K, D + 1]:
 * loss_out double [K] = f_k, grad_out fp32 [K, D + 1] = its gradient (weights, then intercept), both device buffers.  Enqueues only. */
int plipmi_probe_loss_grad(plipmi_handle h, const float* X, int N, int D, const int32_t* y, int K, const float* pos_w,
                           const float* neg_w, float alpha, const float* WB, double* loss_out, float* grad_out, void* stream);

/* Kernel-level entries of the kernels AROUND the GEMMs (csrc/tower_kernels.hip, csrc/head_kernels.hip, csrc/setup_kernels.hip, csrc/attention_probs.hip), for tests/test_gpu_small_kernels.py:
 * each checks its arguments on the host (PLIPMI_ERR_INVALID before any launch), runs the engine's own launcher on `stream` and returns.
 * dtype / y_dtype are PLIPMI_F32 | PLIPMI_BF16 | PLIPMI_F16 (16-bit buffers as raw uint16); "planes" = the split residual form
 * {hi uint16 [rows, D], lo = the blocked 8-bit remainder plane, ((rows + 15) / 16) * 16 * D bytes}; st = fp32 [rows, D / 64, 2]
 * per-64-column partials {sum, centred M2}.  All pointers are device buffers; nothing here synchronises. */

/* probs fp32 [B, H, S, S] = softmax(q k^T + causal + key mask) from qkv [B*S, 3*64*H] (scale folded into q), as HF's eager attention:
 * masked entries exactly 0, a row with no live key all 0.  key_mask int64 [B, S] or NULL.  1 <= S <= 1024. */
int plipmi_attention_probs(int dtype, const void* qkv, float* probs, int B, int S, int H, int causal, const int64_t* key_mask,
                           void* stream);
/* The summary kernels behind the attention-summary entry of plipmi.h (csrc/attention_summary.hip) on the same qkv, under the same masks:
 *   out fp32 [B, H, S] = row rows[b] of P[b, h] (rows int32 [B], each in [0, S)) -- the bits plipmi_attention_probs writes there;
 *   R_out fp32 [B, S, S] = (1/2 mean_h P[b, h] + 1/2 I) . R_in[b], all fp32, head sum in the order h = 0 .. H-1, product summed over
 *   k = 0 .. S-1; R_in == NULL: the identity (the bits an explicit identity gives).  R_out must not be R_in.  B <= 65535. */
int plipmi_attention_pooled_rows(int dtype, const void* qkv, const int32_t* rows, float* out, int B, int S, int H, int causal,
                                 const int64_t* key_mask, void* stream);
int plipmi_attention_rollout_step(int dtype, const void* qkv, const float* R_in, float* R_out, int B, int S, int H, int causal,
                                  const int64_t* key_mask, void* stream);
/* y [rows, D] (y_dtype, contiguous) = LayerNorm(x[r * x_row_stride : + D]) * g + b.  D % 4 == 0, D <= 2048, x_row_stride % 4 == 0 and
 * >= D, x 16-byte aligned.  y may be x itself for fp32 rows of stride D. */
int plipmi_layernorm(const float* x, size_t x_row_stride, const float* g, const float* b, void* y, int y_dtype, int rows, int D,
                     float eps, void* stream);
/* the same rows written as planes of `dtype` (16-bit) plus their statistics partials.  D % 64 == 0, D <= 2048. */
int plipmi_layernorm_emit(int dtype, const float* x, const float* g, const float* b, void* hi, void* lo, float* st, int rows, int D,
                          float eps, void* stream);
/* the weight fold of the 16-bit engines: Wf [rows, K] (dtype) = pre * (W * g, rows centred), c2 [rows] = pre * (W . b + bias).  K % 4 == 0. */
int plipmi_fold_ln(int dtype, const float* W, const float* bias, const float* g, const float* b, void* Wf, float* c2, int rows, int K,
                   float pre, void* stream);
/* token + position rows tok[ids[b, s]] + pos[s] as planes + statistics.  packed = 0: every row, [B*S, D] (eos_id, cu, rowmap, m unused).
 * packed = 1: the pack plan first -- len[b] = EOS position + 1 (eos_id == 2 or < 0: first arg-max of the ids, else the first eos_id, 0
 * if absent), cu int32 [B + 1] = exclusive prefix sums, rowmap int32 [B*S] = (b << 8) | s of each packed row, m int32 [1] = cu[B] --,
 * then rows 0 .. m-1 only.  bad_id: NULL or an int32 flag raised by an id outside [0, vocab).  D % 64 == 0; packed: S <= 256. */
int plipmi_text_embed_emit(int dtype, int packed, const int64_t* ids, const float* tok, const float* pos, void* hi, void* lo, float* st,
                           int B, int S, int D, int vocab, int eos_id, int32_t* cu, int32_t* rowmap, int32_t* m, int32_t* bad_id,
                           void* stream);
/* the pooled row of x fp32 [B, S, D] (ids == NULL: row 0, else the caption's EOS row by the rule above) through LayerNorm and
 *   mode 0: the projection Wt [D, P] (transposed weights), optionally L2-normalised -> out [B, P]   (D <= 2048, P <= 1024)
 *   mode 1: nothing more -> out [B, D]                                                               (D % 4 == 0, D <= 2048) */
int plipmi_pool_rows(int mode, const float* x, int B, int S, int D, const int64_t* ids, int eos_id, const float* ln_w, const float* ln_b,
                     float eps, const float* Wt, int P, int normalize, float* out, void* stream);
/* the pooled row's attention output (att [rows, D], dtype) and residual row (planes -> fp32) copied to attp [B, D] / xp [B, D].
 * cu == NULL: rows are [B, S]; cu int32 [B + 1]: packed rows, sample b's pooled row is cu[b + 1] - 1.  D % 8 == 0. */
int plipmi_pool_gather(int dtype, const void* att, const void* hi, const void* lo, int B, int S, int D, const int64_t* ids, int eos_id,
                       const int32_t* cu, void* attp, float* xp, void* stream);
/* C [M, N] = scale * A [M, K] . W [N, K]^T, the exact-fp32 split-K MFMA kernel of the projection heads and the logits.  N, K % 32 == 0. */
int plipmi_head_gemm(const float* A, const float* W, float* C, int M, int N, int K, float scale, void* stream);

/* The table kernel of the ragged resize (csrc/resize_ragged.hip) on its own, one axis resampled from in_size to out_size pixels:
 * Pillow's 8-bit bicubic tables for outputs first .. first + count -- bounds int32 [count, 2] = (first input index, taps), coef int32
 * [count, ksize] 22-bit fixed-point weights, zero past the taps (device buffers) -- to compare, integer for integer, with
 * plip_amd/preprocess.py resample_coeffs.  in_size / out_size <= 64, ksize >= 2 * ceil(2 * max(in_size / out_size, 1)) + 1. */
int plipmi_resize_ragged_tables(int in_size, int out_size, int first, int count, int ksize, int32_t* bounds, int32_t* coef,
                                void* stream);

/* Kernel-level entries of the vision front end (csrc/towers.hip vision_embed) and of the two mechanisms the packed-caption path rests on,
 * for tests/test_gpu_front_end.py.  As above: arguments checked on the host (PLIPMI_ERR_INVALID before any launch), then the engine's own
 * launcher on `stream`; all pointers are device buffers; nothing synchronises. */

/* The unfold pass: out [B * (H / patch) * (W / patch), Kpad] (dtype) = row (b, gi, gj), column (c, u, v) of the pixels, zeros in columns
 * 3 * patch^2 .. Kpad.  from_u8 = 0: src fp32 NCHW [B, 3, H, W]; 1: src uint8 HWC tiles [B, H, W, 3], CLIP-normalised.  The grid floors.
 * Kpad >= 3 * patch^2, Kpad % 4 == 0, src and out 16-byte aligned. */
int plipmi_unfold_patches(int dtype, int from_u8, const void* src, void* out, int B, int H, int W, int patch, int Kpad, void* stream);
/* x fp32 [B, tokens, D]: row 0 of every image = cls [D] + pos [D] (the position table's first row); the other rows are not touched.
 * D % 4 == 0, tokens >= 1. */
int plipmi_cls_rows(const float* cls, const float* pos, float* x, int B, int tokens, int D, void* stream);
/* The patch GEMM (gemm.h EPI_PATCH): C fp32 [B * (np + 1), N], token row img * (np + 1) + 1 + p = A[img * np + p, :K] . W[n, :K] +
 * pos[1 + p, n]; A [M = B * np, lda], W [N, ldw] (dtype), pos fp32 [np + 1, N].  CLS rows are not touched.  variant as plipmi_gemm_nt
 * (-1 the cost model, 0 .. a tile, -2 the naive kernel, -3 the small-M split-K kernel: 16-bit types, N % 64 == 0, K % 256 == 0).
 * M % np == 0, N % 4 == 0, lda / ldw >= K and multiples of 16 bytes. */
int plipmi_gemm_patch(int dtype, int variant, int M, int N, int K, const void* A, int lda, const void* W, int ldw, const float* pos,
                      int np, void* C, void* stream);
/* The same rows from the patch GEMM with im2col on load (gemm.h ADDR 2 / 3, the ring tile), at ANY batch: exactly one of pixels (fp32
 * NCHW [B, 3, H, W_px]) / tiles (uint8 HWC [B, H, W_px, 3]); W [N, 3 * patch^2] (dtype), pos fp32 [np + 1, N], C fp32 [B * (np + 1), N]
 * with np = (H / patch) * (W_px / patch).  16-bit dtype, patch 16 or 32, W_px % 4 == 0, N % 256 == 0, every buffer below 4 GiB. */
int plipmi_gemm_patch_gather(int dtype, const float* pixels, const uint8_t* tiles, const void* W, const float* pos, float* C, int B,
                             int H, int W_px, int patch, int N, void* stream);
/* plipmi_gemm_nt_ln with the live row count on the device (GemmParams.m_dev, the packed text tower): rows 0 .. min(*m_dev, M) - 1 are
 * computed, M only sizes the grid, nothing past the live rows is written.  variant -1 or a tile (the naive and the small-M kernels do
 * not read m_dev: -2 / -3 are refused). */
int plipmi_gemm_nt_ln_rows(int dtype, int mode, int variant, int M, int N, int K, const void* A, const void* W, const float* bias,
                           const float* stats, int ns, float eps, void* C, void* xb_out, float* st_out, const int32_t* m_dev,
                           void* stream);
/* plipmi_attention on packed rows: cu int32 [B + 1], caption b owns rows cu[b] .. cu[b + 1] - 1 of qkv / out (1 <= its length <= S);
 * key_mask keeps its [B, S] layout.  impl 1 and S <= 128 only (the short-sequence MFMA kernel). */
int plipmi_attention_packed(int dtype, int impl, const void* qkv, void* out, int B, int S, int H, int causal, const int64_t* key_mask,
                            const int32_t* cu, void* stream);

/* The attention entries with the head size as an argument (tests/test_gpu_attention_head_dim.py): plipmi_attention,
 * plipmi_attention_probs, plipmi_attention_pooled_rows and plipmi_attention_rollout_step over qkv [B*S, 3 * H * head_dim] (q | k | v, head
 * h at columns h * head_dim ..; 1/sqrt(head_dim) already folded into q), out [B*S, H * head_dim].  head_dim = 64 is the entry without
 * the argument, the same kernels; 72 .. 128 in steps of 8 run the padded-head kernels of the same units
 * (csrc/attention.hip; csrc/attention_mfma.hip: impl 1 is one chunked kernel for every S; csrc/attention_probs.hip,
 * csrc/attention_summary.hip).  Anything else is refused with
 * PLIPMI_ERR_INVALID and a message that names head_dim.  Every other argument and every result as documented for the entry above. */
int plipmi_attention_hd(int dtype, int impl, const void* qkv, void* out, int B, int S, int H, int head_dim, int causal,
                        const int64_t* key_mask, void* stream);
int plipmi_attention_probs_hd(int dtype, const void* qkv, float* probs, int B, int S, int H, int head_dim, int causal,
                              const int64_t* key_mask, void* stream);
int plipmi_attention_pooled_rows_hd(int dtype, const void* qkv, const int32_t* rows, float* out, int B, int S, int H, int head_dim,
                                    int causal, const int64_t* key_mask, void* stream);
int plipmi_attention_rollout_step_hd(int dtype, const void* qkv, const float* R_in, float* R_out, int B, int S, int H, int head_dim,
                                     int causal, const int64_t* key_mask, void* stream);

/* The scores kernel behind the token-similarity entry of plipmi.h (csrc/token_scores.hip) on its own, for tests/test_gpu_token_similarity.py:
 * out fp32 [M, C] = scale * <E[m] / |E[m]|, T[c] / |T[c]|> for E fp32 [M, P] and T fp32 [C, P] (rows of any norm, no epsilon); softmax != 0:
 * the max-subtracted softmax of those values over c.  P % 32 == 0, 32 <= P <= 1024; 1 <= C <= 64; E and T 16-byte aligned device buffers.
 * Anything else is PLIPMI_ERR_INVALID before any launch; M == 0 launches nothing.  Nothing synchronises. */
int plipmi_token_scores(const float* E, int M, int P, const float* T, int C, float scale, int softmax, float* out, void* stream);

/* One evaluation of the softmax probe's objective (csrc/probe_softmax.hip; arguments as plipmi_softmax_fit in plipmi.h) at WB [C, D + 1],
 * for tests/test_gpu_softmax_probe.py: loss_out double [1] = f, grad_out fp32 [C, D + 1] = its gradient (weights, then intercept), both
 * device buffers.  Enqueues only. */
int plipmi_softmax_loss_grad(plipmi_handle h, const float* X, int N, int D, const int32_t* y, int C, const float* class_w, float alpha,
                             const float* WB, double* loss_out, float* grad_out, void* stream);

/* The update step of k-means alone (csrc/kmeans.hip; limits as plipmi_kmeans_fit in plipmi.h), for tests/test_gpu_kmeans.py: from
 * labels int32 [N] and scores fp32 [N] to sums fp32 [K, D], counts int32 [K], reps int32 [K] (the member with the largest score, ties to
 * the lower row, -1 for an empty cluster) and inertia double [1] = sum_i d_i in the given metric (the argument the distance needs: d_i
 * is |x_i|^2 - 2 s_i or 1 - s_i).  A row whose label is outside [0, K) belongs to no cluster and adds nothing.  Device buffers;
 * deterministic; enqueues only. */
int plipmi_kmeans_update(plipmi_handle h, const float* X, int N, int D, const int32_t* labels, const float* scores, int K, int metric,
                         float* sums, int32_t* counts, int32_t* reps, double* inertia, void* stream);

/* The exact percentile of the stain fit alone (csrc/stain.hip), for tests/test_gpu_stain.py: keys fp32 [S, n] on the device, S segments
 * of n keys, a NaN = an absent key -> out double [S, Q] = numpy's default (linear) percentile q_host[i] (HOST doubles in [0, 100],
 * 1 <= Q <= 8) of the present keys of each segment (NaN for a segment without any), counts int32 [S] (may be NULL) = the present keys.
 * The order statistics are selected exactly (radix select on the order-preserving integer image of a key); the interpolation is fp64.
 * workspace: as many bytes as plipmi.h's plipmi_stain_workspace gives for (S, 1, n, 1), 16-byte aligned.  Device buffers; deterministic; enqueues only; S == 0
 * launches nothing; anything else outside these limits is PLIPMI_ERR_INVALID before any launch. */
int plipmi_stain_percentile(plipmi_handle h, const float* keys, int S, int n, const double* q_host, int Q, double* out, int32_t* counts,
                            void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PLIPMI_TEST_H */
