// kernels.h -- the one interface header of the kernels around the GEMMs: every launcher, grouped by the unit that defines it.
#pragma once
#include "common.h"

namespace plipmi {

// dtype codes used by the launchers: 0 = fp32, 1 = bf16, 2 = f16 (same as PLIPMI_F32 / PLIPMI_BF16 / PLIPMI_F16)

// ===== tower_kernels.hip -- what a tower forward or one of its tap entries launches =====
// y[r,:] = LayerNorm(x[r*x_row_stride : +D]) * g + b ; y is fp32 or bf16, contiguous [rows, D].
// One wavefront per row, statistics in fp32 (two-pass, values held in registers).
hipError_t launch_layernorm(const float* x, size_t x_row_stride, const float* g, const float* b, void* y, int y_dtype,
                            int rows, int D, float eps, hipStream_t s);

// LayerNorm folded into the GEMMs (16-bit engines, gemm.h EPI_*_LN): the one LayerNorm pass a tower keeps -- fp32 rows in,
// the normalised rows out as the split residual stream (common.h split_f32<H>: hi = the 16-bit operand plane [rows, D],
// lo = the 8-bit remainder plane in its blocked layout, lo_plane_bytes(rows, D) bytes) plus their statistics partials st [rows, D/64, 2]
// (D % 64 == 0).  dtype (1 = bf16, 2 = f16) selects H.
hipError_t launch_layernorm_emit(const float* x, const float* g, const float* b, void* hi, void* lo, float* st, int rows, int D,
                                 float eps, int dtype, hipStream_t s);
// the two planes [rows, D] back to plain fp32 (D % 8 == 0)
hipError_t launch_join_planes(const void* hi, const void* lo, float* x, size_t rows, int D, int dtype, hipStream_t s);
// {hi, lo} planes [rows, D] from one 16-bit operand type's split format to the other's (1 bf16, 2 f16), in place (one rounding of the remainder)
hipError_t launch_recode_planes(void* hi, void* lo, size_t rows, int D, int from_dtype, int to_dtype, hipStream_t s);

// pixels fp32 [B,3,H,W] -> patch rows [B*np, Kpad] (dtype), column (c,u,v), zero padded to Kpad.  The grid is
// (H / patch) x (W / patch), row-major; pixels past it are not read (HF's strided conv floors the same way).
hipError_t launch_unfold_patches(const float* pixels, void* out, int out_dtype, int B, int H, int W, int patch, int Kpad,
                                 hipStream_t s);
// Same unfold for raw tiles: uint8 [B,H,W,3] (HWC, what PIL / np.asarray give) with the CLIP normalisation
// (u8/255 - mean[c]) / std[c] of reproducibility/embedders/transform.py:45-52 fused in.
hipError_t launch_unfold_patches_u8(const uint8_t* tiles, void* out, int out_dtype, int B, int H, int W, int patch,
                                    int Kpad, hipStream_t s);

// x[b,0,:] = class_embedding + pos[0,:]   (token rows 1.. are written by the patch GEMM epilogue)
hipError_t launch_cls_rows(const float* cls, const float* pos, float* x, int B, int tokens, int D, hipStream_t s);

// x[b,s,:] = tok[ids[b,s],:] + pos[s,:].  An id outside [0,vocab) is clamped for the lookup and raises *bad_id (a flag
// in host-visible memory; nullptr = no report): the reference's lookup raises there (plip.py:68)
hipError_t launch_text_embed(const int64_t* ids, const float* tok, const float* pos, float* x, int B, int S, int D,
                             int vocab, int* bad_id, hipStream_t s);
// token + position embedding with the same by-products (text tower's first block).  bad_id: see launch_text_embed
hipError_t launch_text_embed_emit(const int64_t* ids, const float* tok, const float* pos, void* hi, void* lo, float* st, int B,
                                  int S, int D, int vocab, int* bad_id, int dtype, hipStream_t s);

// Pooled head: row = CLS (ids == nullptr) or the EOS row of each caption, then
// LayerNorm -> bias-free projection (Wt is the projection TRANSPOSED: [D, P]) -> optional L2 normalise.
hipError_t launch_pool_head(const float* x, int S, int D, const int64_t* ids, int eos_id, const float* ln_w,
                            const float* ln_b, float eps, const float* Wt, int P, float* out, int B, int normalize,
                            hipStream_t s);

// pooled row of every sample (CLS when ids == nullptr, else the caption's EOS row): attention output (bf16) and residual
// row (hi/lo planes -> fp32) copied to compact [B, D] buffers -- the inputs of the last block's pooled-row-only
// out_proj / fc1 / fc2
// cu != nullptr: packed rows, the pooled row of sample b is its last one, cu[b+1]-1
hipError_t launch_pool_gather(const void* att, const void* hi, const void* lo, int S, int D, const int64_t* ids, int eos_id,
                              void* attp, float* xp, int B, int dtype, hipStream_t s, const int* cu = nullptr);

// Packed captions (text tower, opt-in): a causal tower's pooled output depends on rows 0 .. EOS only, so the rows past a
// caption's EOS token need not exist.  One workgroup: len[b] = eos_position(ids[b]) + 1, cu = exclusive prefix sums
// [B+1], rowmap[r] = (b << 8) | t for packed row r (S <= 256), *m_dev = cu[B] = live rows.
hipError_t launch_text_pack(const int64_t* ids, int B, int S, int eos_id, int* cu, int* rowmap, int* m_dev, hipStream_t s);
// token + position embedding of the packed rows (split planes + statistics partials, as launch_text_embed_emit)
hipError_t launch_text_embed_emit_packed(const int64_t* ids, const float* tok, const float* pos, void* hi, void* lo, float* st,
                                         const int* rowmap, const int* m_dev, int max_rows, int S, int D, int vocab,
                                         int* bad_id, int dtype, hipStream_t s);

// Pooled row (CLS, or the EOS row of each caption) -> LayerNorm -> fp32 [B, D]; the projection itself then
// runs on the fp32 MFMA GEMM (used when P % 128 == 0, i.e. every real CLIP/PLIP head).
hipError_t launch_pool_layernorm(const float* x, int S, int D, const int64_t* ids, int eos_id, const float* ln_w,
                                 const float* ln_b, float eps, float* out, int B, hipStream_t s);

hipError_t launch_l2_normalize(float* x, int N, int D, hipStream_t s);
// C[M,N] = A[M,K] . W[N,K]^T, exact fp32 MFMA, split-K over the four waves of a 32x32-tile workgroup (N, K % 32 == 0)
// (also the MFMA form of the logits: C = scale * A . W^T; exchanging A and W gives the bit-exact transpose)
hipError_t launch_head_gemm(const float* A, const float* W, float* C, int M, int N, int K, hipStream_t s, float scale = 1.0f);

// rows [B] int32 = the row of each sample that the heads pool: 0 (ids == nullptr, CLS) or the caption's EOS row by the rule of
// launch_pool_layernorm / launch_pool_gather (tower_kernels.hip eos_position)
hipError_t launch_pooled_row_index(const int64_t* ids, int S, int eos_id, int* rows, int B, hipStream_t s);

// ===== head_kernels.hip -- on finished embeddings, or in front of the image entry; none of it inside a tower forward =====
// logits_per_image[i,j] = scale*<img_i,txt_j>; optional transpose output and per-row first arg-max.
hipError_t launch_logits(const float* img, int Ni, const float* txt, int Nt, int D, float scale, float* lpi,
                         float* lpt, int32_t* argmax, hipStream_t s);
// out[i] = first arg-max of row i of x [N, M]
hipError_t launch_row_argmax(const float* x, int N, int M, int32_t* out, hipStream_t s);
hipError_t launch_topk(const float* scores, int N, int M, int k, int64_t* idx, hipStream_t s);
// streaming top-k: fold the panel scores[rows, 0:ncols] (row stride ld, global column offset col0) into the running
// per-row lists vals/idx [rows, k] (descending; ties: lower index first); init before the first panel, finish after the last
constexpr int kTopkMaxK = 1024;
hipError_t launch_topk_init(float* vals, int64_t* idx, size_t n, hipStream_t s);
hipError_t launch_topk_merge(const float* scores, size_t ld, int rows, int ncols, int64_t col0, int k, float* vals,
                             int64_t* idx, hipStream_t s);
hipError_t launch_topk_finish(int64_t* idx, size_t n, hipStream_t s);

// Pillow-exact 8-bit bicubic resize + centre crop of uint8 HWC images (tables from plip_amd/preprocess.py):
// src [B,H,W,3] -> tmp [B,R,n,3] (rows r0..r0+R of the source, horizontally resampled) -> dst [B,n,n,3]
hipError_t launch_resize_crop_u8(const uint8_t* src, int B, int H, int W, int n, const int* xb, const int* xk, int xks,
                                 int left, const int* yb, const int* yk, int yks, int top, int r0, int R,
                                 uint8_t* tmp, uint8_t* dst, hipStream_t s);

hipError_t launch_occupy(unsigned long long wall_clock_ticks, hipStream_t s);   // one workgroup, no memory traffic (plipmi_streams_overlap)

// ===== setup_kernels.hip -- once per handle (plipmi_create, plipmi_clone_resolution) =====
// weight folding at plipmi_create (the weights' side of launch_layernorm_emit's fold): Wf[n,:] = H(pre * (W[n,:] * g - mean_k(W[n,:] * g))), c2[n] = pre * (W[n,:].b + bias[n])
hipError_t launch_fold_ln(const float* W, const float* bias, const float* g, const float* b, void* Wf, float* c2, int rows,
                          int K, float pre, int dtype, hipStream_t s);

// Position table for another patch grid (CLIPVisionEmbeddings.interpolate_pos_encoding): row 0 (CLS) copied, the n0 x n0
// patch rows of src [1 + n0*n0, D] resampled to gh x gw rows of dst [1 + gh*gw, D] -- torch.nn.functional.interpolate(mode =
// "bicubic", align_corners = False) in fp32: A = -0.75, src = (n0 / g) * (dst + 0.5) - 0.5, taps clamped to the border,
// x pass then y pass.  dst must not alias src.
hipError_t launch_resample_pos(const float* src, float* dst, int n0, int gh, int gw, int D, hipStream_t s);

// dst[r, 0:cols] = (T)(scale * src[r, 0:cols]), dst[r, cols:dst_ld] = 0   (weight packing)
hipError_t launch_convert(const float* src, void* dst, int dst_dtype, int rows, int cols, int dst_ld, float scale,
                          hipStream_t s);
// dst[c, r] = src[r, c]   fp32 (projection weights -> [D, P])
hipError_t launch_transpose(const float* src, float* dst, int rows, int cols, hipStream_t s);
hipError_t launch_scale_copy(const float* src, float* dst, int n, float scale, hipStream_t s);

// ===== attention.hip (the dispatcher and the fp32 VALU kernel), attention_mfma.hip (the MFMA kernels; their device pieces, shared
// with qkv_attention.hip, are in attention_mfma_dev.h) =====
// Multi-head attention over the fused qkv buffer [B*S, 3*D] (D = H * head; q | k | v, head h at columns h*head..), the
// 1/sqrt(head) scale already folded into q.  out [B*S, D].  causal: key j <= query i.  key_mask: int64 [B,S] or nullptr.
//   head  64, or 72 .. 128 in steps of 8 (attention_head_ok).  The kernels are instantiated at attention_head_pad(head) columns: 64,
//         or a padded size whose columns past the head are zeros in LDS, never read from memory and never stored
//   impl 0 = exact fp32 VALU kernel (any dtype, S <= 1024), 1 = MFMA kernel (dtype bf16 or f16; heads other than 64: one chunked
//   kernel for every S)
//   cu (impl 1, S <= 128, head 64): packed rows -- sample b owns rows cu[b] .. cu[b+1]-1 of qkv / out (its first cu[b+1]-cu[b]
//   positions; the rest of its S positions do not exist); key_mask keeps its [B, S] layout
inline bool attention_head_ok(int head) { return head >= 64 && head <= 128 && head % 8 == 0; }
inline int attention_head_pad(int head) { return head == 64 ? 64 : head <= 96 ? 96 : 128; }
hipError_t launch_attention(const void* qkv, void* out, int dtype, int B, int S, int H, int head, int causal,
                            const int64_t* key_mask, int impl, hipStream_t s, const int* cu = nullptr);

// ===== qkv_attention.hip =====
// The text tower's LayerNorm-folded q/k/v projection with the attention in its epilogue (qkv_attention.hip): one launch, no
// `qkv` tensor in memory.  A = the residual stream's operand plane [B*S, D], W / c2 = the folded q | k | v weights [3D, D] and
// biases, stats = the rows' LayerNorm partials [B*S, D/64, 2]; out = attention output [B*S, D], bit-identical to
// gemm.h EPI_BIAS_LN followed by launch_attention(impl 1).  16-bit dtypes, 65 .. 80 tokens, D = 64 H.
bool qkv_attention_supports(int dtype, int B, int S, int H, int D);
bool qkv_attention_pays(int B, int H, int num_cus);   // enough workgroups to fill the chip: below, the two kernels are faster
hipError_t launch_qkv_attention(int dtype, const void* A, const void* W, const float* c2, const float* stats, float ln_inv_d,
                                float ln_eps, void* out, int B, int S, int H, int causal, const int64_t* key_mask, hipStream_t s,
                                unsigned long long* trace = nullptr /* test hook: in-kernel timeline, 8 x u64 per workgroup */);

// ===== attention_probs.hip =====
// Attention probabilities of HF's eager attention (attention_probs.hip, plipmi_encode_tower_outputs only): fp32
// probs [B, H, S, S] = softmax(q k^T + mask) from the same qkv buffer (dtype 0 fp32, 1 bf16, 2 f16), the same causal / key_mask
// rules; masked entries exactly 0, a row with no live key all 0.  S <= 1024.  head as launch_attention.
hipError_t launch_attention_probs(const void* qkv, float* probs, int dtype, int B, int S, int H, int head, int causal,
                                  const int64_t* key_mask, hipStream_t s);

// ===== attention_summary.hip =====
// Attention summaries (attention_summary.hip, plipmi_encode_attention_summary only), from the same qkv buffer and under the same
// causal / key_mask rules as launch_attention_probs, whose probabilities they reproduce bit for bit.  S <= 1024.
//   pooled rows:  out fp32 [B, H, S] = row rows[b] of P[b, h]
//   rollout step: R_out [B, S, S] = (1/2 mean_h P[b, h] + 1/2 I) . R_in[b] in fp32 (head sum h = 0 .. H-1, product k = 0 .. S-1);
//                 R_in == nullptr: the identity.  R_out must not be R_in.  Dynamic LDS: attention_rollout_lds_bytes(S).
//                 pooled_out != nullptr (with rows): the step also stores the pooled rows, [B, H, S], the bits of the kernel above
//   rollout row:  out [B, S] = row rows[b] of R[b]
size_t attention_rollout_lds_bytes(int S, int head = 64);
hipError_t launch_attention_pooled_rows(const void* qkv, const int* rows, float* out, int dtype, int B, int S, int H, int head, int causal,
                                        const int64_t* key_mask, hipStream_t s);
hipError_t launch_attention_rollout_step(const void* qkv, const float* R_in, float* R_out, int dtype, int B, int S, int H, int head,
                                         int causal, const int64_t* key_mask, hipStream_t s, const int* rows = nullptr,
                                         float* pooled_out = nullptr);
hipError_t launch_attention_rollout_row(const float* R, const int* rows, float* out, int B, int S, hipStream_t s);

// ===== token_scores.hip =====
// Dense image-text scores (token_scores.hip, plipmi_encode_token_similarity only): out fp32 [M, C] = scale * <E[m] / |E[m]|, T[c] / |T[c]|>
// for token embeddings E [M, P] and text embeddings T [C, P] (fp32, rows of any norm, no epsilon), softmax != 0: the max-subtracted
// softmax of those values over c.  P % 32 == 0, 32 <= P <= 1024; 1 <= C <= kTokenSimMaxC; E and T 16-byte aligned.  Fixed-order sums: a
// row's bits depend on neither M nor the row's place.  Dynamic LDS: token_scores_lds_bytes(P) (sixteen text rows at a time).
constexpr int kTokenSimMaxC = 64;
size_t token_scores_lds_bytes(int P);
hipError_t launch_token_scores(const float* E, int M, int P, const float* T, int C, float scale, int softmax, float* out, hipStream_t s);

// ===== probe.hip =====
// Linear-probe head (probe.hip): one loss-and-gradient evaluation of the K one-vs-rest logistic problems at WB [K, D + 1] (weights,
// then intercept) over X [N, D] fp32 with int32 labels y: problem k's positive label is class_base + k, its sample weights pos_w[k] /
// neg_w[k].  `scratch` (probe_scratch_bytes) holds the per-workgroup partials and the results: *grad = fp32 [K, D + 1], *loss =
// double [K] point into it.  D % 4 == 0, D <= 1024, K <= 64, X 16-byte aligned.  Deterministic: fixed-order reductions.
// The embedding tile and what this unit, probe_softmax.hip and kmeans.hip share around it are in probe_tile.h and probe_fit_*.inc.
size_t probe_scratch_bytes(int N, int D, int K, size_t* grad_off, size_t* loss_off, size_t* partl_off);
hipError_t launch_probe_loss_grad(const float* X, int N, int D, const int32_t* y, const float* WB, int K, const float* pos_w,
                                  const float* neg_w, int class_base, float alpha, char* scratch, float** grad, double** loss,
                                  hipStream_t s);
// decision [N, K] = X W^T + b (may be nullptr) and pred [N] = first arg-max over the K problems (K == 1: z > 0)
hipError_t launch_probe_predict(const float* X, int N, int D, const float* WB, int K, float* decision, int32_t* pred, hipStream_t s);

// ===== probe_softmax.hip =====
// Softmax (multinomial) linear probe: one loss-and-gradient evaluation of f(W, b) = (1/N) sum_i cw[y_i] (logsumexp_k z_ik - z_iy) +
// alpha/2 |W|_F^2 at WB [C, D + 1] over X [N, D] fp32 with int32 labels y; class_w fp32 [C] or nullptr = ones; a label outside [0, C)
// gives its row weight 0.  `scratch` (softmax_scratch_bytes) holds the per-workgroup partials, the rows' statistics (C > 16) and the
// results: *grad = fp32 [C, D + 1], *loss = double [1] point into it.  D % 4 == 0, D <= 1024, 2 <= C <= 64, X 16-byte aligned.
// C <= 16: X is read once; else 1 + ceil(C / 16) times.  Deterministic: fixed-order reductions.
size_t softmax_scratch_bytes(int N, int D, int C);
hipError_t launch_softmax_loss_grad(const float* X, int N, int D, const int32_t* y, const float* WB, int C, const float* class_w,
                                    float alpha, char* scratch, float** grad, double** loss, hipStream_t s);

// ===== resize_ragged.hip =====
// The same resize + crop for a RAGGED batch (resize_ragged.hip): B images of their own sizes packed in src at offsets[b] (device int64),
// hw int32 [B, 2] on the device; geometry, coefficient tables and the layout of the intermediate are computed on the device inside
// `workspace` (resize_ragged.h RaggedLayout L, sized and checked by the caller on the host).  dst [B, n, n, 3].
struct RaggedLayout;
hipError_t launch_resize_crop_ragged(const uint8_t* src, size_t src_bytes, const int64_t* offsets, const int32_t* hw, int B, int n,
                                     int rule, int ks, int max_cap, void* workspace, const RaggedLayout& L, uint8_t* dst,
                                     hipStream_t s);
// its table kernel alone, one axis: outputs first .. first + count of `in` -> `out` pixels; bounds int32 [count, 2], coef int32 [count, ks]
hipError_t launch_ragged_tables(int in, int out, int first, int count, int ks, int* bounds, int* coef, hipStream_t s);

}  // namespace plipmi
