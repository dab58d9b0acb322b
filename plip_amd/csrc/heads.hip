// heads.hip -- what runs on embeddings and images outside the towers: L2 normalisation, logits, top-k and the streaming
// similarity top-k, the Pillow-exact resize entries, and the linear-probe drivers (probe.hip, probe_softmax.hip, probe_solver.h): both
// fits run probe_solve below, K machines of D + 1 variables or one machine of C (D + 1).
#include <algorithm>
#include <cmath>

#include "handle.h"
#include "probe_solver.h"
#include "resize_ragged.h"

using namespace plipmi;

namespace {

struct ProbeSolve { int evals, conv, worst; double gmax; };      // worst: the machine with the largest final gradient, gmax

// The solver loop of both probe fits: `machines` L-BFGS machines (probe_solver.h) of n variables each on WB_inout [machines][n], one
// loss per machine.  Every pass evaluates all the current trial points in one call, eval(&grad, &loss), which leaves device pointers to
// fp32 [machines][n] and double [machines]; the trial points travel through WB_inout itself, which ends holding every machine's final
// point.  Fills info_out (may be nullptr) and *out; a machine that did not converge (out->conv < machines) is the caller's to report.
template <typename Eval>
int probe_solve(plipmi_handle h, int machines, int n, int max_iter, float gtol, float* WB_inout, plipmi_probe_info* info_out,
                hipStream_t s, Eval&& eval, ProbeSolve* out) {
  const size_t wb_bytes = (size_t)machines * n * 4;
  RUN(h->probe_host.reserve(2 * align_up(wb_bytes, 256) + align_up((size_t)machines * 8, 256), s));
  float* wb_h = reinterpret_cast<float*>(h->probe_host.data());
  float* g_h = reinterpret_cast<float*>(h->probe_host.data() + align_up(wb_bytes, 256));
  double* l_h = reinterpret_cast<double*>(h->probe_host.data() + 2 * align_up(wb_bytes, 256));

  HIP_TRY(hipMemcpyAsync(wb_h, WB_inout, wb_bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (size_t i = 0; i < (size_t)machines * n; ++i)
    if (!std::isfinite(wb_h[i])) return fail(PLIPMI_ERR_INVALID, "the starting point WB_inout holds a non-finite value");
  std::vector<ProbeLbfgs> prob(machines);
  for (int k = 0; k < machines; ++k) prob[k].init(wb_h + (size_t)k * n, n, max_iter, (double)gtol);
  *out = ProbeSolve{0, 0, -1, 0.0};
  for (;;) {
    for (int k = 0; k < machines; ++k) prob[k].trial(wb_h + (size_t)k * n);
    HIP_TRY(hipMemcpyAsync(WB_inout, wb_h, wb_bytes, hipMemcpyHostToDevice, s));
    bool all_done = true;
    for (int k = 0; k < machines; ++k) all_done = all_done && prob[k].done;
    if (all_done) break;
    float* grad; double* loss;
    RUN(eval(&grad, &loss));
    HIP_TRY(hipMemcpyAsync(g_h, grad, wb_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(l_h, loss, (size_t)machines * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    ++out->evals;
    for (int k = 0; k < machines; ++k) prob[k].feed(l_h[k], g_h + (size_t)k * n);
  }
  HIP_TRY(hipStreamSynchronize(s));
  int iters = 0;
  for (int k = 0; k < machines; ++k) {
    iters = std::max(iters, prob[k].iters);
    out->conv += prob[k].converged ? 1 : 0;
    if (prob[k].gnorm >= out->gmax) { out->gmax = prob[k].gnorm; out->worst = k; }
  }
  if (info_out) {
    memset(info_out, 0, sizeof(*info_out));
    info_out->iterations = iters; info_out->evaluations = out->evals; info_out->converged = out->conv; info_out->grad_norm = out->gmax;
    for (int k = 0; k < machines; ++k) info_out->loss[k] = prob[k].f;
  }
  return PLIPMI_OK;
}

}  // namespace

extern "C" {

int plipmi_l2_normalize(plipmi_handle h, float* x, int N, int D, void* stream) {
  if (!h || !x || N < 0 || D <= 0) return fail(PLIPMI_ERR_INVALID, "bad argument");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Scope sc(h, s, "l2_normalize", 0, (double)N * D * 8);
  HIP_TRY(launch_l2_normalize(x, N, D, s));
  return PLIPMI_OK;
}

int plipmi_logits(plipmi_handle h, const float* img, int Ni, const float* txt, int Nt, int D, float scale,
                  float* logits_per_image, float* logits_per_text, int32_t* argmax_per_image, void* stream) {
  if (!h || !img || !txt || !logits_per_image || Ni < 0 || Nt < 0 || D <= 0) return fail(PLIPMI_ERR_INVALID, "bad argument");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (Ni == 0 || Nt == 0) return PLIPMI_OK;
  // Exact-fp32 MFMA whenever the shape tiles (the bs=256 logits of CLIPModel.forward do): one 32x32 tile per workgroup,
  // K split over its four waves.  logits_per_text is the same kernel with the operands exchanged -- products commute
  // and the k order is identical, so it is bit-for-bit the transpose.  Other shapes (e.g. 10 class prompts) take the
  // scalar-FMA kernel.
  if (D % 32 == 0 && Nt % 32 == 0 && (!logits_per_text || Ni % 32 == 0) && (size_t)Ni * Nt <= (1u << 22)) {
    { Scope sc(h, s, "logits_mfma", 2.0 * Ni * (double)Nt * D, ((double)Ni + Nt) * D * 4 + (double)Ni * Nt * 4);
      HIP_TRY(launch_head_gemm(img, txt, logits_per_image, Ni, Nt, D, s, scale)); }
    if (logits_per_text) {
      Scope sc(h, s, "logits_mfma", 2.0 * Ni * (double)Nt * D, ((double)Ni + Nt) * D * 4 + (double)Ni * Nt * 4);
      HIP_TRY(launch_head_gemm(txt, img, logits_per_text, Nt, Ni, D, s, scale)); }
    if (argmax_per_image) { Scope sc(h, s, "row_argmax", 0, (double)Ni * Nt * 4); HIP_TRY(launch_row_argmax(logits_per_image, Ni, Nt, argmax_per_image, s)); }
    return PLIPMI_OK;
  }
  Scope sc(h, s, "logits", 2.0 * Ni * (double)Nt * D, ((double)Ni + Nt) * D * 4 + (double)Ni * Nt * 4);
  HIP_TRY(launch_logits(img, Ni, txt, Nt, D, scale, logits_per_image, logits_per_text, argmax_per_image, s));
  return PLIPMI_OK;
}

int plipmi_topk(plipmi_handle h, const float* scores, int N, int M, int k, int64_t* idx, void* stream) {
  if (!h || !scores || !idx || N < 0 || M <= 0 || k <= 0 || k > M) return fail(PLIPMI_ERR_INVALID, "bad argument (need 0 < k <= M)");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Scope sc(h, s, "topk", 0, (double)N * M * 4 * k);
  HIP_TRY(launch_topk(scores, N, M, k, idx, s));
  return PLIPMI_OK;
}

int plipmi_resize_crop_u8(plipmi_handle h, const uint8_t* src, int B, int H, int W, int n_px, const int32_t* xbounds,
                          const int32_t* xcoef, int xksize, int left, const int32_t* ybounds, const int32_t* ycoef,
                          int yksize, int top, int row0, int nrows, uint8_t* tmp, uint8_t* dst, void* stream) {
  if (!h || B < 0 || H <= 0 || W <= 0 || n_px <= 0) return fail(PLIPMI_ERR_INVALID, "bad argument");
  if (B == 0) return PLIPMI_OK;
  if (!src || !tmp || !dst) return fail(PLIPMI_ERR_INVALID, "null src/tmp/dst");
  if ((xbounds == nullptr) != (xcoef == nullptr) || (ybounds == nullptr) != (ycoef == nullptr))
    return fail(PLIPMI_ERR_INVALID, "bounds and coefficients come in pairs");
  if (row0 < 0 || nrows <= 0 || row0 + nrows > H) return fail(PLIPMI_ERR_INVALID, "rows [%d, %d) outside the %d-row image", row0, row0 + nrows, H);
  if (!xbounds && (left < 0 || left + n_px > W)) return fail(PLIPMI_ERR_INVALID, "crop columns outside the image");
  if (!ybounds && (top < row0 || top + n_px > row0 + nrows)) return fail(PLIPMI_ERR_INVALID, "crop rows outside the staged rows");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Scope sc(h, s, "resize_crop_u8", 0, (double)B * ((double)nrows * W * 3 + 2.0 * nrows * n_px * 3 + (double)n_px * n_px * 3));
  HIP_TRY(launch_resize_crop_u8(src, B, H, W, n_px, xbounds, xcoef, xksize, left, ybounds, ycoef, yksize, top, row0, nrows,
                                tmp, dst, s));
  return PLIPMI_OK;
}

size_t plipmi_resize_ragged_workspace(const int32_t* hw_host, int B, int n_px, int ksize) {
  if (!hw_host || B <= 0 || n_px <= 0 || ksize <= 0) return 0;
  return rr_layout(hw_host, B, n_px, ksize).total;
}

int plipmi_resize_crop_u8_ragged(plipmi_handle h, const uint8_t* src, size_t src_bytes, const int64_t* offsets, const int32_t* hw,
                                 const int64_t* offsets_host, const int32_t* hw_host, int B, int n_px, int crop_rule, int ksize,
                                 void* workspace, size_t workspace_bytes, uint8_t* dst, void* stream) {
  if (!h || B < 0 || n_px <= 0 || (crop_rule != 0 && crop_rule != 1)) return fail(PLIPMI_ERR_INVALID, "bad argument");
  if (B == 0) return PLIPMI_OK;
  if (B > kRaggedMaxBatch) return fail(PLIPMI_ERR_INVALID, "%d images in one call (at most %d)", B, kRaggedMaxBatch);
  if (!src || !offsets || !hw || !offsets_host || !hw_host || !workspace || !dst)
    return fail(PLIPMI_ERR_INVALID, "null src/offsets/hw/workspace/dst");
  int need = 0, max_cap = 0;
  const char* why = "";
  if (const int bad = rr_check_batch(offsets_host, hw_host, B, n_px, crop_rule, src_bytes, &need, &max_cap, &why))
    return fail(PLIPMI_ERR_INVALID, "image %d (%d x %d at byte %lld of %zu): %s", bad - 1, hw_host[2 * (bad - 1)],
                hw_host[2 * (bad - 1) + 1], (long long)offsets_host[bad - 1], src_bytes, why);
  if (ksize < need) return fail(PLIPMI_ERR_INVALID, "ksize %d is below the %d taps of the batch's largest scale", ksize, need);
  const RaggedLayout L = rr_layout(hw_host, B, n_px, ksize);
  if (workspace_bytes < L.total)
    return fail(PLIPMI_ERR_INVALID, "workspace of %zu bytes, plipmi_resize_ragged_workspace asks for %zu", workspace_bytes, L.total);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  double bytes = (double)B * n_px * n_px * 3;
  for (int b = 0; b < B; ++b) bytes += (double)hw_host[2 * b] * hw_host[2 * b + 1] * 3;
  Scope sc(h, s, "resize_crop_u8_ragged", 0, bytes + 2.0 * (double)L.tmp_bytes);
  HIP_TRY(launch_resize_crop_ragged(src, src_bytes, offsets, hw, B, n_px, crop_rule, ksize, max_cap, workspace, L, dst, s));
  return PLIPMI_OK;
}

int plipmi_similarity_topk(plipmi_handle h, const float* keys, int Nq, const float* space, int Ns, int D, int k,
                           int64_t* idx, float* vals, void* stream) {
  if (!h || Nq < 0 || Ns <= 0 || D <= 0) return fail(PLIPMI_ERR_INVALID, "bad argument");
  if (Nq > 0 && (!keys || !space || !idx)) return fail(PLIPMI_ERR_INVALID, "null keys/space/idx");
  if (k <= 0 || k > Ns || k > kTopkMaxK)
    return fail(PLIPMI_ERR_INVALID, "need 0 < k <= min(Ns, %d), got k=%d Ns=%d", kTopkMaxK, k, Ns);
  if (D % 32) return fail(PLIPMI_ERR_INVALID, "embedding width %d must be a multiple of 32", D);
  if (Nq == 0) return PLIPMI_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // panel geometry: [QB queries] x [PB space vectors] of fp32 scores at a time (<= 128 MiB), never [Nq, Ns]
  const int PB = (int)std::min<size_t>(8192, align_up((size_t)Ns, 256));
  const int QB = std::min(Nq, 4096);
  const int tail = Ns % PB;  // the last panel is staged zero-padded so the GEMM's N stays a whole number of tiles
  const size_t sc_bytes = align_up((size_t)QB * PB * 4, 256);
  const size_t tl_bytes = tail ? align_up((size_t)align_up((size_t)tail, 256) * D * 4, 256) : 0;
  const size_t vl_bytes = vals ? 0 : align_up((size_t)QB * k * 4, 256);
  const size_t need = sc_bytes + tl_bytes + vl_bytes;
  RUN(h->sim_ws.reserve(need, s));
  float* scores = reinterpret_cast<float*>(h->sim_ws.data());
  float* tail_w = reinterpret_cast<float*>(h->sim_ws.data() + sc_bytes);
  float* own_vals = reinterpret_cast<float*>(h->sim_ws.data() + sc_bytes + tl_bytes);
  const int tail_n = (int)align_up((size_t)tail, 256);
  if (tail) {
    HIP_TRY(hipMemsetAsync(tail_w, 0, (size_t)tail_n * D * 4, s));
    HIP_TRY(hipMemcpyAsync(tail_w, space + (size_t)(Ns - tail) * D, (size_t)tail * D * 4, hipMemcpyDeviceToDevice, s));
  }
  for (int q0 = 0; q0 < Nq; q0 += QB) {
    const int rows = std::min(QB, Nq - q0);
    float* v = vals ? vals + (size_t)q0 * k : own_vals;
    int64_t* ix = idx + (size_t)q0 * k;
    HIP_TRY(launch_topk_init(v, ix, (size_t)rows * k, s));
    for (int p0 = 0; p0 < Ns; p0 += PB) {
      const int cols = std::min(PB, Ns - p0);
      const bool is_tail = cols < PB;
      const GemmParams p = make_params(keys + (size_t)q0 * D, is_tail ? tail_w : space + (size_t)p0 * D, scores, nullptr, rows,
                                       is_tail ? tail_n : PB, D, D, D, PB);
      const char* name = "gemm_nt";
      { Scope sc(h, s, name, 2.0 * rows * (double)p.N * D, ((double)rows * D + (double)p.N * D + (double)rows * p.N) * 4);
        const int rc = gemm_launch(PLIPMI_F32, EPI_SCALE, p.N % 256 == 0 && rows > 128 ? -1 : 1, p, s, &name);
        sc.rename(name);
        if (rc != 0) return fail(PLIPMI_ERR_HIP, "similarity gemm failed: %s", hipGetErrorString((hipError_t)rc)); }
      { Scope sc(h, s, "topk_merge", 0, (double)rows * cols * 4);
        HIP_TRY(launch_topk_merge(scores, (size_t)PB, rows, cols, (int64_t)p0, k, v, ix, s)); }
    }
    HIP_TRY(launch_topk_finish(ix, (size_t)rows * k, s));
  }
  return PLIPMI_OK;
}

// ---- linear-probe head (probe.hip, probe_solver.h) ----------------------------------------------------------------------
static int probe_check(plipmi_handle h, const void* X, int N, int D, const void* WB, int K) {
  if (!h || !X || !WB) return fail(PLIPMI_ERR_INVALID, "null handle / X / WB");
  if (K < 1 || K > PLIPMI_PROBE_MAX_K) return fail(PLIPMI_ERR_INVALID, "need 1 <= K <= %d problems, got %d", PLIPMI_PROBE_MAX_K, K);
  return check_embeddings("", X, N, D);
}
static int probe_check_fit(const void* y, const void* pos_w, const void* neg_w, float alpha) {
  if (!y || !pos_w || !neg_w) return fail(PLIPMI_ERR_INVALID, "null y / pos_w / neg_w");
  if (!std::isfinite(alpha) || alpha <= 0.f) return fail(PLIPMI_ERR_INVALID, "alpha must be finite and > 0, got %g", (double)alpha);
  return PLIPMI_OK;
}
static int probe_scratch(plipmi_handle h, int N, int D, int K, hipStream_t s) {
  size_t go, lo, po;
  return h->probe_ws.reserve(probe_scratch_bytes(N, D, K, &go, &lo, &po), s);
}
static int probe_eval(plipmi_handle h, const float* X, int N, int D, const int32_t* y, int K, const float* pos_w, const float* neg_w,
                      float alpha, const float* WB, float** grad, double** loss, hipStream_t s) {
  Scope sc(h, s, "probe_loss_grad", 4.0 * N * (double)D * 16 * ((K + 15) / 16), (double)N * D * 4 * ((K + 15) / 16));
  HIP_TRY(launch_probe_loss_grad(X, N, D, y, WB, K, pos_w, neg_w, K == 1 ? 1 : 0, alpha, h->probe_ws.data(), grad, loss, s));
  return PLIPMI_OK;
}

int plipmi_probe_loss_grad(plipmi_handle h, const float* X, int N, int D, const int32_t* y, int K, const float* pos_w,
                           const float* neg_w, float alpha, const float* WB, double* loss_out, float* grad_out, void* stream) {
  RUN(probe_check(h, X, N, D, WB, K));
  RUN(probe_check_fit(y, pos_w, neg_w, alpha));
  if (!loss_out || !grad_out) return fail(PLIPMI_ERR_INVALID, "null loss_out / grad_out");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  RUN(probe_scratch(h, N, D, K, s));
  float* grad; double* loss;
  RUN(probe_eval(h, X, N, D, y, K, pos_w, neg_w, alpha, WB, &grad, &loss, s));
  HIP_TRY(hipMemcpyAsync(grad_out, grad, (size_t)K * (D + 1) * 4, hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemcpyAsync(loss_out, loss, (size_t)K * 8, hipMemcpyDeviceToDevice, s));
  return PLIPMI_OK;
}

int plipmi_probe_fit(plipmi_handle h, const float* X, int N, int D, const int32_t* y, int K, const float* pos_w, const float* neg_w,
                     float alpha, int max_iter, float gtol, float* WB_inout, plipmi_probe_info* info_out, void* stream) {
  RUN(probe_check(h, X, N, D, WB_inout, K));
  RUN(probe_check_fit(y, pos_w, neg_w, alpha));
  if (max_iter < 1 || !std::isfinite(gtol) || gtol <= 0.f) return fail(PLIPMI_ERR_INVALID, "need max_iter >= 1 and a finite gtol > 0");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  RUN(probe_scratch(h, N, D, K, s));
  // K machines of D + 1 variables: the one-vs-rest problems are independent
  ProbeSolve r;
  RUN(probe_solve(h, K, D + 1, max_iter, gtol, WB_inout, info_out, s, [&](float** grad, double** loss) {
    return probe_eval(h, X, N, D, y, K, pos_w, neg_w, alpha, WB_inout, grad, loss, s);
  }, &r));
  if (r.conv != K)
    return fail(PLIPMI_ERR_NOT_CONVERGED, "probe fit: %d of %d problems did not reach |grad|_inf <= %g within %d iterations "
                "(largest %g, problem %d, %d evaluations); WB holds the best point found", K - r.conv, K, (double)gtol, max_iter, r.gmax,
                r.worst, r.evals);
  return PLIPMI_OK;
}

int plipmi_probe_predict(plipmi_handle h, const float* X, int N, int D, const float* WB, int K, float* decision, int32_t* pred,
                         void* stream) {
  RUN(probe_check(h, X, N, D, WB, K));
  if (!pred) return fail(PLIPMI_ERR_INVALID, "null pred");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Scope sc(h, s, "probe_predict", 2.0 * N * (double)D * K, (double)N * D * 4);
  HIP_TRY(launch_probe_predict(X, N, D, WB, K, decision, pred, s));
  return PLIPMI_OK;
}

// ---- softmax linear probe (probe_softmax.hip, probe_solver.h) ------------------------------------------------------------------
static int softmax_check(plipmi_handle h, const void* X, int N, int D, const void* y, int C, float alpha, const void* WB) {
  if (!h || !X || !y || !WB) return fail(PLIPMI_ERR_INVALID, "null handle / X / y / WB");
  if (C < 2 || C > PLIPMI_PROBE_MAX_K) return fail(PLIPMI_ERR_INVALID, "need 2 <= C <= %d classes, got %d", PLIPMI_PROBE_MAX_K, C);
  RUN(check_embeddings("", X, N, D));
  if (!std::isfinite(alpha) || alpha <= 0.f) return fail(PLIPMI_ERR_INVALID, "alpha must be finite and > 0, got %g", (double)alpha);
  return PLIPMI_OK;
}
static int softmax_eval(plipmi_handle h, const float* X, int N, int D, const int32_t* y, int C, const float* class_w, float alpha,
                        const float* WB, float** grad, double** loss, hipStream_t s) {
  const int passes = C <= 16 ? 1 : 1 + (C + 15) / 16;      // over X
  Scope sc(h, s, "softmax_loss_grad", 4.0 * N * (double)D * 16 * ((C + 15) / 16) + (C > 16 ? 2.0 * N * (double)D * C : 0.0),
           (double)N * D * 4 * passes);
  HIP_TRY(launch_softmax_loss_grad(X, N, D, y, WB, C, class_w, alpha, h->probe_ws.data(), grad, loss, s));
  return PLIPMI_OK;
}

int plipmi_softmax_loss_grad(plipmi_handle h, const float* X, int N, int D, const int32_t* y, int C, const float* class_w, float alpha,
                             const float* WB, double* loss_out, float* grad_out, void* stream) {
  RUN(softmax_check(h, X, N, D, y, C, alpha, WB));
  if (!loss_out || !grad_out) return fail(PLIPMI_ERR_INVALID, "null loss_out / grad_out");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  RUN(h->probe_ws.reserve(softmax_scratch_bytes(N, D, C), s));
  float* grad; double* loss;
  RUN(softmax_eval(h, X, N, D, y, C, class_w, alpha, WB, &grad, &loss, s));
  HIP_TRY(hipMemcpyAsync(grad_out, grad, (size_t)C * (D + 1) * 4, hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemcpyAsync(loss_out, loss, 8, hipMemcpyDeviceToDevice, s));
  return PLIPMI_OK;
}

int plipmi_softmax_fit(plipmi_handle h, const float* X, int N, int D, const int32_t* y, int C, const float* class_w, float alpha,
                       int max_iter, float gtol, float* WB_inout, plipmi_probe_info* info_out, void* stream) {
  RUN(softmax_check(h, X, N, D, y, C, alpha, WB_inout));
  if (max_iter < 1 || !std::isfinite(gtol) || gtol <= 0.f) return fail(PLIPMI_ERR_INVALID, "need max_iter >= 1 and a finite gtol > 0");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  RUN(h->probe_ws.reserve(softmax_scratch_bytes(N, D, C), s));
  // ONE machine over all C (D + 1) variables: the classes are coupled
  ProbeSolve r;
  RUN(probe_solve(h, 1, C * (D + 1), max_iter, gtol, WB_inout, info_out, s, [&](float** grad, double** loss) {
    return softmax_eval(h, X, N, D, y, C, class_w, alpha, WB_inout, grad, loss, s);
  }, &r));
  if (!r.conv)
    return fail(PLIPMI_ERR_NOT_CONVERGED, "softmax fit: did not reach |grad|_inf <= %g within %d iterations (now %g, %d evaluations); "
                "WB holds the best point found", (double)gtol, max_iter, r.gmax, r.evals);
  return PLIPMI_OK;
}

}  // extern "C"
