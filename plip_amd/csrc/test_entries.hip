// test_entries.hip -- the kernel-level entries and process-wide A/B hooks of include/plipmi_test.h: arguments checked here, then
// the engine's own launcher.  (plipmi_debug_hidden and plipmi_probe_loss_grad sit with the drivers they exercise: towers.hip, heads.hip.)
#include "handle.h"
#include "resize_ragged.h"

using namespace plipmi;

extern "C" {

int plipmi_gemm_nt(int dtype, int epilogue, int variant, int M, int N, int K, const void* A, const void* W,
                   const float* bias, float alpha, void* C, void* stream) {
  return plipmi_gemm_nt_traced(dtype, epilogue, variant, M, N, K, A, W, bias, alpha, C, nullptr, stream);
}

int plipmi_gemm_nt_traced(int dtype, int epilogue, int variant, int M, int N, int K, const void* A, const void* W,
                          const float* bias, float alpha, void* C, uint64_t* trace, void* stream) {
  if (!valid_dtype(dtype)) return fail(PLIPMI_ERR_INVALID, "bad dtype");
  if (epilogue < 0 || epilogue > EPI_SCALE) return fail(PLIPMI_ERR_INVALID, "epilogue must be 0..3");
  if (M < 0 || N <= 0 || K <= 0 || !A || !W || !C) return fail(PLIPMI_ERR_INVALID, "bad shape / null pointer");
  if (epilogue != EPI_SCALE && !bias) return fail(PLIPMI_ERR_INVALID, "bias required for this epilogue");
  GemmParams p = make_params(A, W, C, bias, M, N, K, K, K, N);
  p.alpha = alpha;
  p.trace = reinterpret_cast<unsigned long long*>(trace);
  const int rc = (variant == -3 && dtype != PLIPMI_F32)     // -3: the small-M split-K kernel (gemm_skinny.hip)
                     ? gemm_launch_skinny(dtype, epilogue, p, reinterpret_cast<hipStream_t>(stream), nullptr)
                     : gemm_launch(dtype, epilogue, variant, p, reinterpret_cast<hipStream_t>(stream), nullptr);
  if (rc != 0) return fail(PLIPMI_ERR_HIP, "gemm launch failed (variant %d, M=%d N=%d K=%d): %s", variant, M, N, K,
                           hipGetErrorString((hipError_t)rc));
  return PLIPMI_OK;
}

}  // extern "C"

// plipmi_gemm_nt_ln / plipmi_gemm_nt_ln_rows: the latter with the live row count on the device
static int gemm_nt_ln_entry(int dtype, int mode, int variant, int M, int N, int K, const void* A, const void* W, const float* bias,
                            const float* stats, int ns, float eps, void* C, void* xb_out, float* st_out, const int* m_dev, void* stream) {
  if (!half_code(dtype)) return fail(PLIPMI_ERR_INVALID, "LayerNorm-folded epilogues are 16-bit-engine forms");
  if (mode < 0 || mode > 4 || M < 0 || N <= 0 || K <= 0 || !A || !W || !C || !bias) return fail(PLIPMI_ERR_INVALID, "bad argument");
  if (mode < 2 && (!stats || ns <= 0)) return fail(PLIPMI_ERR_INVALID, "mode 0/1 need the row statistics");
  if (mode < 2 && ns % 2) return fail(PLIPMI_ERR_INVALID, "mode 0/1 read the statistics two slices at a time: ns = %d must be even (LayerNorm widths are multiples of 128)", ns);
  if (mode >= 2 && (!xb_out || !st_out || N % kLnSlice)) return fail(PLIPMI_ERR_INVALID, "mode 2/3 need xb_out, st_out and N %% 64 == 0");
  if (mode == 4 && variant == -3)    // gemm_skinny.hip's EPI_RESID_SPLIT ignores planes_other: it would write dtype's own format
    return fail(PLIPMI_ERR_INVALID, "mode 4 at variant -3: the small-M kernel writes the planes in the type it reads them in (the engine re-codes them in enter_block instead)");
  GemmParams p = make_params(A, W, C, bias, M, N, K, K, K, N);
  p.m_dev = m_dev;
  p.ln_stats = stats; p.ln_ns = ns; p.ln_inv_d = ns > 0 ? 1.0f / (float)(ns * kLnSlice) : 0.f; p.ln_eps = eps;
  p.xb_out = xb_out; p.st_out = st_out;
  if (mode >= 3) { p.lo_io = C; p.C = nullptr; p.planes_other = mode == 4; }
  const int epi = mode == 0 ? EPI_BIAS_LN : mode == 1 ? EPI_QGELU_LN : mode == 2 ? EPI_RESID_EMIT : EPI_RESID_SPLIT;
  const int rc = variant == -3 ? gemm_launch_skinny(dtype, epi, p, reinterpret_cast<hipStream_t>(stream), nullptr)
                               : gemm_launch(dtype, epi, variant, p, reinterpret_cast<hipStream_t>(stream), nullptr);
  if (rc != 0) return fail(PLIPMI_ERR_HIP, "gemm launch failed (LN mode %d, variant %d, M=%d N=%d K=%d): %s", mode, variant, M, N, K,
                           hipGetErrorString((hipError_t)rc));
  return PLIPMI_OK;
}

extern "C" {

int plipmi_gemm_nt_ln(int dtype, int mode, int variant, int M, int N, int K, const void* A, const void* W, const float* bias,
                      const float* stats, int ns, float eps, void* C, void* xb_out, float* st_out, void* stream) {
  return gemm_nt_ln_entry(dtype, mode, variant, M, N, K, A, W, bias, stats, ns, eps, C, xb_out, st_out, nullptr, stream);
}
int plipmi_gemm_nt_ln_rows(int dtype, int mode, int variant, int M, int N, int K, const void* A, const void* W, const float* bias,
                           const float* stats, int ns, float eps, void* C, void* xb_out, float* st_out, const int32_t* m_dev,
                           void* stream) {
  if (!m_dev) return fail(PLIPMI_ERR_INVALID, "null m_dev (plipmi_gemm_nt_ln is the form without a device-side row count)");
  if (variant < -1) return fail(PLIPMI_ERR_INVALID, "variant %d does not read a device-side row count: -1 or a tile", variant);
  return gemm_nt_ln_entry(dtype, mode, variant, M, N, K, A, W, bias, stats, ns, eps, C, xb_out, st_out, m_dev, stream);
}

int plipmi_gemm_nt_gelu(int dtype, int ln, int variant, int M, int N, int K, const void* A, const void* W, const float* bias,
                        const float* stats, int ns, float eps, void* C, void* stream) {
  if (!valid_dtype(dtype)) return fail(PLIPMI_ERR_INVALID, "bad dtype");
  if (ln != 0 && ln != 1) return fail(PLIPMI_ERR_INVALID, "ln must be 0 (gelu(A.W^T + bias)) or 1 (gelu(rstd * A.W^T + bias))");
  if (ln && !half_code(dtype)) return fail(PLIPMI_ERR_INVALID, "LayerNorm-folded epilogues are 16-bit-engine forms");
  if (M < 0 || N <= 0 || K <= 0 || !A || !W || !C || !bias) return fail(PLIPMI_ERR_INVALID, "bad shape / null pointer");
  if (ln && (!stats || ns <= 0)) return fail(PLIPMI_ERR_INVALID, "ln = 1 needs the row statistics");
  if (ln && ns % 2) return fail(PLIPMI_ERR_INVALID, "ln = 1 reads the statistics two slices at a time: ns = %d must be even (LayerNorm widths are multiples of 128)", ns);
  if (ln && variant == -2) return fail(PLIPMI_ERR_INVALID, "ln = 1 at variant -2: the naive checker has no LayerNorm-folded form");
  if (variant == -3 && !half_code(dtype)) return fail(PLIPMI_ERR_INVALID, "variant -3: the small-M kernel takes 16-bit operands");
  GemmParams p = make_params(A, W, C, bias, M, N, K, K, K, N);
  if (ln) { p.ln_stats = stats; p.ln_ns = ns; p.ln_inv_d = 1.0f / (float)(ns * kLnSlice); p.ln_eps = eps; }
  const int epi = ln ? EPI_GELU_LN : EPI_BIAS_GELU;
  const int rc = variant == -3 ? gemm_launch_skinny(dtype, epi, p, reinterpret_cast<hipStream_t>(stream), nullptr)
                               : gemm_launch(dtype, epi, variant, p, reinterpret_cast<hipStream_t>(stream), nullptr);
  if (rc != 0) return fail(PLIPMI_ERR_HIP, "gemm launch failed (gelu, ln %d, variant %d, M=%d N=%d K=%d): %s", ln, variant, M, N, K,
                           hipGetErrorString((hipError_t)rc));
  return PLIPMI_OK;
}

int plipmi_attention(int dtype, int impl, const void* qkv, void* out, int B, int S, int H, int causal,
                     const int64_t* key_mask, void* stream) {
  return plipmi_attention_hd(dtype, impl, qkv, out, B, S, H, 64, causal, key_mask, stream);
}
// what every *_hd entry refuses in front of its launcher: a head size no attention kernel is built for
static int check_head_dim(int head_dim) {
  if (!attention_head_ok(head_dim))
    return fail(PLIPMI_ERR_INVALID, "head_dim = %d: the attention kernels take 64, or 72 .. 128 in steps of 8", head_dim);
  return PLIPMI_OK;
}
int plipmi_attention_hd(int dtype, int impl, const void* qkv, void* out, int B, int S, int H, int head_dim, int causal,
                        const int64_t* key_mask, void* stream) {
  if (!valid_dtype(dtype) || !qkv || !out || B < 0 || S <= 0 || H <= 0)
    return fail(PLIPMI_ERR_INVALID, "bad argument");
  RUN(check_head_dim(head_dim));
  hipError_t e = launch_attention(qkv, out, dtype, B, S, H, head_dim, causal, key_mask, impl, reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess)
    return fail(PLIPMI_ERR_HIP, "attention launch (impl %d, S=%d, head_dim=%d) failed: %s", impl, S, head_dim, hipGetErrorString(e));
  return PLIPMI_OK;
}

int plipmi_attention_packed(int dtype, int impl, const void* qkv, void* out, int B, int S, int H, int causal, const int64_t* key_mask,
                            const int32_t* cu, void* stream) {
  if (!half_code(dtype) || !qkv || !out || !cu || B < 0 || S <= 0 || H <= 0) return fail(PLIPMI_ERR_INVALID, "bad argument (16-bit dtype, qkv, out, cu non-null)");
  if (impl != 1 || S > 128) return fail(PLIPMI_ERR_INVALID, "packed rows are a form of the short-sequence MFMA kernel: impl 1, S <= 128 (got impl %d, S=%d)", impl, S);
  hipError_t e = launch_attention(qkv, out, dtype, B, S, H, 64, causal, key_mask, impl, reinterpret_cast<hipStream_t>(stream), cu);
  if (e != hipSuccess) return fail(PLIPMI_ERR_HIP, "packed attention launch (S=%d) failed: %s", S, hipGetErrorString(e));
  return PLIPMI_OK;
}

int plipmi_gemm_nt_ld(int dtype, int epilogue, int variant, int M, int N, int K, const void* A, int lda, const void* W,
                      int ldw, const float* bias, float alpha, void* C, void* stream) {
  if (!valid_dtype(dtype)) return fail(PLIPMI_ERR_INVALID, "bad dtype");
  if (epilogue < 0 || epilogue > EPI_SCALE) return fail(PLIPMI_ERR_INVALID, "epilogue must be 0..3");
  const int per16 = dtype == PLIPMI_F32 ? 4 : 8;
  if (M < 0 || N <= 0 || K <= 0 || !A || !W || !C || lda < K || ldw < K || lda % per16 || ldw % per16)
    return fail(PLIPMI_ERR_INVALID, "bad shape / leading dimension (must be >= K and a multiple of 16 bytes)");
  if (epilogue != EPI_SCALE && !bias) return fail(PLIPMI_ERR_INVALID, "bias required for this epilogue");
  GemmParams p = make_params(A, W, C, bias, M, N, K, lda, ldw, N);
  p.alpha = alpha;
  const int rc = gemm_launch(dtype, epilogue, variant, p, reinterpret_cast<hipStream_t>(stream), nullptr);
  if (rc != 0) return fail(PLIPMI_ERR_HIP, "gemm launch failed (variant %d, M=%d N=%d K=%d): %s", variant, M, N, K,
                           hipGetErrorString((hipError_t)rc));
  return PLIPMI_OK;
}

int plipmi_test_force_gemm_tile(int variant) {
  if (!gemm_force_tile(variant)) return fail(PLIPMI_ERR_INVALID, "tile %d: -1 (cost model), -2 (naive checker) or 0 .. %d", variant, gemm_num_variants() - 1);
  ++g_hook_epoch;
  return PLIPMI_OK;
}
int plipmi_test_remap_gemm_tile(int from, int to) {
  if (!gemm_remap_tile(from, to)) return fail(PLIPMI_ERR_INVALID, "remap %d -> %d: tiles are 0 .. %d (to = -1 clears)", from, to, gemm_num_variants() - 1);
  ++g_hook_epoch;
  return PLIPMI_OK;
}
int plipmi_test_fused_qkv_attention(int mode) {
  if (mode < 0 || mode > 2) return fail(PLIPMI_ERR_INVALID, "fused q/k/v + attention mode %d: 0 (two kernels), 1 (product rule), 2 (fused wherever it applies)", mode);
  g_fuse_qkv_attention = mode;
  ++g_hook_epoch;
  return PLIPMI_OK;
}
int plipmi_test_patch_gather(int on) {
  if (on != 0 && on != 1) return fail(PLIPMI_ERR_INVALID, "patch gather %d: 0 (unfold pass) or 1 (im2col on load where it applies)", on);
  g_patch_gather = on;
  ++g_hook_epoch;
  return PLIPMI_OK;
}
void plipmi_test_reset_hooks(void) {
  g_fuse_qkv_attention = 1;
  g_patch_gather = 1;
  gemm_reset_overrides();
  ++g_hook_epoch;
}
int plipmi_qkv_attention(int dtype, const void* A, const void* W, const float* c2, const float* stats, int ns, float eps, void* out,
                         int B, int S, int H, int causal, const int64_t* key_mask, uint64_t* trace, void* stream) {
  if (!A || !W || !c2 || !stats || !out || ns <= 0 || ns * kLnSlice != H * 64) return fail(PLIPMI_ERR_INVALID, "bad argument");
  if (!qkv_attention_supports(dtype, B, S, H, H * 64))
    return fail(PLIPMI_ERR_INVALID, "the fused q/k/v + attention kernel takes 16-bit operands, 65 .. 80 tokens, widths of 64 H (a multiple of 128)");
  HIP_TRY(launch_qkv_attention(dtype, A, W, c2, stats, 1.0f / (float)(ns * kLnSlice), eps, out, B, S, H, causal, key_mask,
                               reinterpret_cast<hipStream_t>(stream), reinterpret_cast<unsigned long long*>(trace)));
  return PLIPMI_OK;
}
int plipmi_resample_pos(const float* src, float* dst, int n0, int gh, int gw, int D, void* stream) {
  if (!src || !dst || src == dst || n0 <= 0 || gh <= 0 || gw <= 0 || D <= 0 || 1 + gh * gw > 1024 * 1024)
    return fail(PLIPMI_ERR_INVALID, "bad argument (src [1 + n0*n0, D], dst [1 + gh*gw, D], distinct)");
  HIP_TRY(launch_resample_pos(src, dst, n0, gh, gw, D, reinterpret_cast<hipStream_t>(stream)));
  return PLIPMI_OK;
}
int plipmi_resize_ragged_tables(int in_size, int out_size, int first, int count, int ksize, int32_t* bounds, int32_t* coef,
                                void* stream) {
  if (in_size < 1 || out_size < 1 || first < 0 || count < 0 || first + count > out_size)
    return fail(PLIPMI_ERR_INVALID, "bad argument (outputs first .. first + count of out_size)");
  if ((double)in_size / (double)out_size > (double)kRaggedMaxRatio || ksize < rr_ksize(in_size, out_size))
    return fail(PLIPMI_ERR_INVALID, "in / out above %d, or ksize %d below the axis's %d taps", kRaggedMaxRatio, ksize,
                rr_ksize(in_size, out_size));
  if (count == 0) return PLIPMI_OK;
  if (!bounds || !coef) return fail(PLIPMI_ERR_INVALID, "null bounds/coef");
  HIP_TRY(launch_ragged_tables(in_size, out_size, first, count, ksize, bounds, coef, reinterpret_cast<hipStream_t>(stream)));
  return PLIPMI_OK;
}

int plipmi_attention_probs(int dtype, const void* qkv, float* probs, int B, int S, int H, int causal, const int64_t* key_mask,
                           void* stream) {
  return plipmi_attention_probs_hd(dtype, qkv, probs, B, S, H, 64, causal, key_mask, stream);
}
int plipmi_attention_probs_hd(int dtype, const void* qkv, float* probs, int B, int S, int H, int head_dim, int causal,
                              const int64_t* key_mask, void* stream) {
  if (!valid_dtype(dtype) || !qkv || !probs || B < 0 || S <= 0 || S > 1024 || H <= 0)
    return fail(PLIPMI_ERR_INVALID, "bad argument (qkv, probs non-null, 1 <= S <= 1024, H >= 1)");
  RUN(check_head_dim(head_dim));
  const hipError_t e = launch_attention_probs(qkv, probs, dtype, B, S, H, head_dim, causal, key_mask, reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail(PLIPMI_ERR_HIP, "attention probabilities launch (S=%d) failed: %s", S, hipGetErrorString(e));
  return PLIPMI_OK;
}
int plipmi_attention_pooled_rows(int dtype, const void* qkv, const int32_t* rows, float* out, int B, int S, int H, int causal,
                                 const int64_t* key_mask, void* stream) {
  return plipmi_attention_pooled_rows_hd(dtype, qkv, rows, out, B, S, H, 64, causal, key_mask, stream);
}
int plipmi_attention_pooled_rows_hd(int dtype, const void* qkv, const int32_t* rows, float* out, int B, int S, int H, int head_dim,
                                    int causal, const int64_t* key_mask, void* stream) {
  if (!valid_dtype(dtype) || !qkv || !rows || !out || B < 0 || B > 65535 || S <= 0 || S > 1024 || H <= 0)
    return fail(PLIPMI_ERR_INVALID, "bad argument (qkv, rows, out non-null, B <= 65535, 1 <= S <= 1024, H >= 1)");
  RUN(check_head_dim(head_dim));
  const hipError_t e = launch_attention_pooled_rows(qkv, rows, out, dtype, B, S, H, head_dim, causal, key_mask, reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail(PLIPMI_ERR_HIP, "pooled attention rows launch (S=%d) failed: %s", S, hipGetErrorString(e));
  return PLIPMI_OK;
}
int plipmi_attention_rollout_step(int dtype, const void* qkv, const float* R_in, float* R_out, int B, int S, int H, int causal,
                                  const int64_t* key_mask, void* stream) {
  return plipmi_attention_rollout_step_hd(dtype, qkv, R_in, R_out, B, S, H, 64, causal, key_mask, stream);
}
int plipmi_attention_rollout_step_hd(int dtype, const void* qkv, const float* R_in, float* R_out, int B, int S, int H, int head_dim,
                                     int causal, const int64_t* key_mask, void* stream) {
  if (!valid_dtype(dtype) || !qkv || !R_out || B < 0 || B > 65535 || S <= 0 || S > 1024 || H <= 0)
    return fail(PLIPMI_ERR_INVALID, "bad argument (qkv, R_out non-null, B <= 65535, 1 <= S <= 1024, H >= 1)");
  if (R_in == R_out) return fail(PLIPMI_ERR_INVALID, "R_out must not be R_in: every tile of a step reads all of R_in");
  RUN(check_head_dim(head_dim));
  const hipError_t e = launch_attention_rollout_step(qkv, R_in, R_out, dtype, B, S, H, head_dim, causal, key_mask, reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail(PLIPMI_ERR_HIP, "attention rollout step launch (S=%d) failed: %s", S, hipGetErrorString(e));
  return PLIPMI_OK;
}
int plipmi_layernorm(const float* x, size_t x_row_stride, const float* g, const float* b, void* y, int y_dtype, int rows, int D,
                     float eps, void* stream) {
  if (!x || !g || !b || !y || rows < 0 || !valid_dtype(y_dtype)) return fail(PLIPMI_ERR_INVALID, "bad argument");
  if (D <= 0 || D % 4 || D > 2048 || x_row_stride % 4 || x_row_stride < (size_t)D)
    return fail(PLIPMI_ERR_INVALID, "LayerNorm width %d / row stride %zu: D %% 4 == 0, D <= 2048, stride %% 4 == 0, stride >= D", D, x_row_stride);
  if (y == (const void*)x && (y_dtype != PLIPMI_F32 || x_row_stride != (size_t)D))
    return fail(PLIPMI_ERR_INVALID, "in place: fp32 rows of stride D only");
  HIP_TRY(launch_layernorm(x, x_row_stride, g, b, y, y_dtype, rows, D, eps, reinterpret_cast<hipStream_t>(stream)));
  return PLIPMI_OK;
}
int plipmi_layernorm_emit(int dtype, const float* x, const float* g, const float* b, void* hi, void* lo, float* st, int rows, int D,
                          float eps, void* stream) {
  if (!half_code(dtype) || !x || !g || !b || !hi || !lo || !st || rows < 0) return fail(PLIPMI_ERR_INVALID, "bad argument");
  if (D <= 0 || D % kLnSlice || D > 2048) return fail(PLIPMI_ERR_INVALID, "width %d: D %% 64 == 0, D <= 2048", D);
  HIP_TRY(launch_layernorm_emit(x, g, b, hi, lo, st, rows, D, eps, dtype, reinterpret_cast<hipStream_t>(stream)));
  return PLIPMI_OK;
}
int plipmi_fold_ln(int dtype, const float* W, const float* bias, const float* g, const float* b, void* Wf, float* c2, int rows, int K,
                   float pre, void* stream) {
  if (!half_code(dtype) || !W || !bias || !g || !b || !Wf || !c2 || rows < 0 || K <= 0 || K % 4)
    return fail(PLIPMI_ERR_INVALID, "bad argument (16-bit dtype, K %% 4 == 0)");
  HIP_TRY(launch_fold_ln(W, bias, g, b, Wf, c2, rows, K, pre, dtype, reinterpret_cast<hipStream_t>(stream)));
  return PLIPMI_OK;
}
int plipmi_text_embed_emit(int dtype, int packed, const int64_t* ids, const float* tok, const float* pos, void* hi, void* lo, float* st,
                           int B, int S, int D, int vocab, int eos_id, int32_t* cu, int32_t* rowmap, int32_t* m, int32_t* bad_id,
                           void* stream) {
  if (!half_code(dtype) || !ids || !tok || !pos || !hi || !lo || !st || B < 0 || S <= 0 || vocab <= 0 || (packed != 0 && packed != 1))
    return fail(PLIPMI_ERR_INVALID, "bad argument");
  if (D <= 0 || D % kLnSlice) return fail(PLIPMI_ERR_INVALID, "width %d: D %% 64 == 0", D);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (!packed) {
    HIP_TRY(launch_text_embed_emit(ids, tok, pos, hi, lo, st, B, S, D, vocab, bad_id, dtype, s));
    return PLIPMI_OK;
  }
  if (!cu || !rowmap || !m) return fail(PLIPMI_ERR_INVALID, "the packed form returns cu [B + 1], rowmap [B * S] and m [1]");
  if (S > 256 || (size_t)(B + 1) * sizeof(int) > 64 * 1024) return fail(PLIPMI_ERR_INVALID, "packing: S <= 256, B + 1 <= 16384 (got S=%d B=%d)", S, B);
  HIP_TRY(launch_text_pack(ids, B, S, eos_id, cu, rowmap, m, s));
  HIP_TRY(launch_text_embed_emit_packed(ids, tok, pos, hi, lo, st, rowmap, m, B * S, S, D, vocab, bad_id, dtype, s));
  return PLIPMI_OK;
}
int plipmi_pool_rows(int mode, const float* x, int B, int S, int D, const int64_t* ids, int eos_id, const float* ln_w, const float* ln_b,
                     float eps, const float* Wt, int P, int normalize, float* out, void* stream) {
  if ((mode != 0 && mode != 1) || !x || !ln_w || !ln_b || !out || B < 0 || S <= 0 || D <= 0) return fail(PLIPMI_ERR_INVALID, "bad argument");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (mode == 0) {
    if (!Wt || P <= 0 || P > 1024 || D > 2048) return fail(PLIPMI_ERR_INVALID, "pooled head: D <= 2048, 1 <= P <= 1024 (got D=%d P=%d)", D, P);
    HIP_TRY(launch_pool_head(x, S, D, ids, eos_id, ln_w, ln_b, eps, Wt, P, out, B, normalize, s));
    return PLIPMI_OK;
  }
  if (D % 4 || D > 2048) return fail(PLIPMI_ERR_INVALID, "pooled LayerNorm: D %% 4 == 0, D <= 2048 (got %d)", D);
  HIP_TRY(launch_pool_layernorm(x, S, D, ids, eos_id, ln_w, ln_b, eps, out, B, s));
  return PLIPMI_OK;
}
int plipmi_pool_gather(int dtype, const void* att, const void* hi, const void* lo, int B, int S, int D, const int64_t* ids, int eos_id,
                       const int32_t* cu, void* attp, float* xp, void* stream) {
  if (!half_code(dtype) || !att || !hi || !lo || !attp || !xp || B < 0 || S <= 0 || D <= 0 || D % 8)
    return fail(PLIPMI_ERR_INVALID, "bad argument (16-bit dtype, D %% 8 == 0)");
  HIP_TRY(launch_pool_gather(att, hi, lo, S, D, ids, eos_id, attp, xp, B, dtype, reinterpret_cast<hipStream_t>(stream), cu));
  return PLIPMI_OK;
}
int plipmi_head_gemm(const float* A, const float* W, float* C, int M, int N, int K, float scale, void* stream) {
  if (!A || !W || !C || M < 0 || N <= 0 || K <= 0 || N % 32 || K % 32) return fail(PLIPMI_ERR_INVALID, "bad argument (N %% 32 == 0, K %% 32 == 0)");
  HIP_TRY(launch_head_gemm(A, W, C, M, N, K, reinterpret_cast<hipStream_t>(stream), scale));
  return PLIPMI_OK;
}
int plipmi_recode_planes(void* hi, void* lo, size_t rows, int D, int from_dtype, int to_dtype, void* stream) {
  if (!hi || !lo || D <= 0 || D % 8) return fail(PLIPMI_ERR_INVALID, "null planes / width not a multiple of 8");
  HIP_TRY(launch_recode_planes(hi, lo, rows, D, from_dtype, to_dtype, reinterpret_cast<hipStream_t>(stream)));
  return PLIPMI_OK;
}

// ---- the vision front end, kernel by kernel (towers.hip vision_embed) --------------------------------------------------------------
int plipmi_unfold_patches(int dtype, int from_u8, const void* src, void* out, int B, int H, int W, int patch, int Kpad, void* stream) {
  if (!valid_dtype(dtype) || (from_u8 != 0 && from_u8 != 1) || !src || !out || B < 0) return fail(PLIPMI_ERR_INVALID, "bad argument");
  if (patch <= 0 || patch > 64 || H < patch || W < patch || H > 16384 || W > 16384)
    return fail(PLIPMI_ERR_INVALID, "patch %d / image %d x %d: 1 <= patch <= 64, at least one patch, sides <= 16384", patch, H, W);
  if (Kpad < 3 * patch * patch || Kpad % 4) return fail(PLIPMI_ERR_INVALID, "Kpad %d: >= 3 * patch^2 = %d and a multiple of 4", Kpad, 3 * patch * patch);
  if (((uintptr_t)src | (uintptr_t)out) % 16) return fail(PLIPMI_ERR_INVALID, "src / out must be 16-byte aligned");
  if ((size_t)B * (H / patch) * (W / patch) > 0x7fffffffull) return fail(PLIPMI_ERR_INVALID, "more than 2^31 - 1 patch rows");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (from_u8) HIP_TRY(launch_unfold_patches_u8(static_cast<const uint8_t*>(src), out, dtype, B, H, W, patch, Kpad, s));
  else HIP_TRY(launch_unfold_patches(static_cast<const float*>(src), out, dtype, B, H, W, patch, Kpad, s));
  return PLIPMI_OK;
}
int plipmi_cls_rows(const float* cls, const float* pos, float* x, int B, int tokens, int D, void* stream) {
  if (!cls || !pos || !x || B < 0 || tokens < 1 || D <= 0 || D % 4) return fail(PLIPMI_ERR_INVALID, "bad argument (tokens >= 1, D %% 4 == 0)");
  if (((uintptr_t)cls | (uintptr_t)pos | (uintptr_t)x) % 16) return fail(PLIPMI_ERR_INVALID, "cls / pos / x must be 16-byte aligned");
  HIP_TRY(launch_cls_rows(cls, pos, x, B, tokens, D, reinterpret_cast<hipStream_t>(stream)));
  return PLIPMI_OK;
}
int plipmi_gemm_patch(int dtype, int variant, int M, int N, int K, const void* A, int lda, const void* W, int ldw, const float* pos,
                      int np, void* C, void* stream) {
  if (!valid_dtype(dtype)) return fail(PLIPMI_ERR_INVALID, "bad dtype");
  const int per16 = dtype == PLIPMI_F32 ? 4 : 8;
  if (M < 0 || N <= 0 || N % 4 || K <= 0 || !A || !W || !C || !pos || lda < K || ldw < K || lda % per16 || ldw % per16)
    return fail(PLIPMI_ERR_INVALID, "bad shape / null pointer / leading dimension (N %% 4 == 0; lda, ldw >= K and multiples of 16 bytes)");
  if (np <= 0 || M % np) return fail(PLIPMI_ERR_INVALID, "np = %d patches per image must be positive and divide M = %d", np, M);
  if (variant < -3) return fail(PLIPMI_ERR_INVALID, "variant %d: -1 (cost model), -2 (naive checker), -3 (small-M split-K kernel) or a tile", variant);
  // -3: what gemm_launch_skinny would refuse is refused here, by name, before anything is launched
  if (variant == -3 && !half_code(dtype)) return fail(PLIPMI_ERR_INVALID, "variant -3: the small-M kernel takes 16-bit operands");
  if (variant == -3 && (!gemm_skinny_supports(EPI_PATCH, M > 0 ? M : 1, N, K) || lda % 8 || ldw % 8))
    return fail(PLIPMI_ERR_INVALID, "variant -3: the small-M kernel needs N %% 64 == 0, K %% 256 == 0 and lda, ldw multiples of 8 (got N=%d K=%d lda=%d ldw=%d)", N, K, lda, ldw);
  GemmParams p = make_params(A, W, C, pos, M, N, K, lda, ldw, N);
  p.np = np;
  const int rc = variant == -3 ? gemm_launch_skinny(dtype, EPI_PATCH, p, reinterpret_cast<hipStream_t>(stream), nullptr)
                               : gemm_launch(dtype, EPI_PATCH, variant, p, reinterpret_cast<hipStream_t>(stream), nullptr);
  if (rc != 0) return fail(PLIPMI_ERR_HIP, "patch gemm launch failed (variant %d, M=%d N=%d K=%d): %s", variant, M, N, K,
                           hipGetErrorString((hipError_t)rc));
  return PLIPMI_OK;
}
int plipmi_gemm_patch_gather(int dtype, const float* pixels, const uint8_t* tiles, const void* W, const float* pos, float* C, int B,
                             int H, int W_px, int patch, int N, void* stream) {
  // what gemm_gather_supports and gemm_launch_gather refuse, without the cost-model clause (this entry runs the ring tile at any batch)
  if (!half_code(dtype)) return fail(PLIPMI_ERR_INVALID, "im2col on load is a 16-bit-engine form");
  if ((pixels != nullptr) == (tiles != nullptr) || !W || !pos || !C || B < 0) return fail(PLIPMI_ERR_INVALID, "bad argument (exactly one of pixels / tiles; W, pos, C non-null)");
  if (patch != 16 && patch != 32) return fail(PLIPMI_ERR_INVALID, "patch %d: the gather takes 16- and 32-pixel patches", patch);
  if (H < patch || W_px < patch || W_px % 4) return fail(PLIPMI_ERR_INVALID, "image %d x %d: at least one patch, width %% 4 == 0", H, W_px);
  if (N <= 0 || N % 256) return fail(PLIPMI_ERR_INVALID, "N = %d: whole 256-column tiles", N);
  const int np = (H / patch) * (W_px / patch), K = 3 * patch * patch;
  const size_t M = (size_t)B * np;
  if ((size_t)B * 3 * H * W_px * 4 >= (1ull << 32) || (M + B + 1) * N * 4 >= (1ull << 32) || (size_t)N * K * 2 >= (1ull << 32))
    return fail(PLIPMI_ERR_INVALID, "pixels, output rows and weights must each stay below 4 GiB (32-bit buffer offsets)");
  // GemmParams as vision_embed fills them (kpad == K for these patch sides)
  GemmParams p = make_params(nullptr, W, C, pos, (int)M, N, K, K, K, N);
  p.np = np;
  p.pix = pixels; p.tiles = tiles; p.img_h = H; p.img_w = W_px; p.patch_log2 = patch == 32 ? 5 : 4;
  const int rc = gemm_launch_gather(dtype, p, reinterpret_cast<hipStream_t>(stream), nullptr);
  if (rc != 0) return fail(PLIPMI_ERR_HIP, "patch GEMM (im2col on load) failed: %s", hipGetErrorString((hipError_t)rc));
  return PLIPMI_OK;
}

int plipmi_token_scores(const float* E, int M, int P, const float* T, int C, float scale, int softmax, float* out, void* stream) {
  if (M < 0) return fail(PLIPMI_ERR_INVALID, "M = %d rows", M);
  if (P < 32 || P > 1024 || P % 32) return fail(PLIPMI_ERR_INVALID, "P = %d: a multiple of 32, 32 .. 1024", P);
  if (C < 1 || C > kTokenSimMaxC) return fail(PLIPMI_ERR_INVALID, "C = %d text rows: 1 .. %d", C, kTokenSimMaxC);
  if (!E || !T || !out) return fail(PLIPMI_ERR_INVALID, "null E / T / out");
  if ((reinterpret_cast<uintptr_t>(E) | reinterpret_cast<uintptr_t>(T)) % 16) return fail(PLIPMI_ERR_INVALID, "E / T must be 16-byte aligned");
  HIP_TRY(launch_token_scores(E, M, P, T, C, scale, softmax, out, reinterpret_cast<hipStream_t>(stream)));
  return PLIPMI_OK;
}

int plipmi_gemm_variant_built(int dtype, int variant) {
  if (!valid_dtype(dtype)) return 0;
  return gemm_variant_is_built(dtype, variant) ? 1 : 0;
}

const char* plipmi_gemm_variant_name(int variant) {
  if (variant < 0 || variant >= gemm_num_variants()) return nullptr;
  return gemm_variant(variant).name;
}

}  // extern "C"
