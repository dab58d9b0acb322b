// gemm.h -- the interface of the NT GEMM: epilogue kinds, launch parameters and the host-side entry points.
//
//   C = epilogue( A[M,K] * W[N,K]^T )         A, W row-major, K contiguous
//
// which is exactly nn.Linear (HF stores Linear weights [out,in]) -- q/k/v, out_proj,
// fc1, fc2 (modeling_clip.py:293-296,343-344), the unfolded patch-embed conv
// (:148-154) and, with A = image embeds / W = text embeds, the logits (:814).
//
// No device code here: the engine side (handle.h) includes this file only.  The kernel is gemm_kernel.h (tile traits
// gemm_tile.h, fill gemm_fill.h, K loops gemm_kloop.h, epilogues gemm_epilogue.h), instantiated per dtype by gemm_inst.h;
// the LDS-DMA / store / MFMA helpers other kernels share are gemm_lds.h.
#pragma once
#include <hip/hip_runtime.h>

namespace plipmi {

enum Epilogue : int {
  EPI_BIAS = 0,        // C(T)   = acc + bias[n]
  EPI_BIAS_QGELU = 1,  // C(T)   = quickgelu(acc + bias[n])
  EPI_BIAS_RESID = 2,  // C(f32) += acc + bias[n]            (in-place residual stream)
  EPI_SCALE = 3,       // C(f32) = alpha * acc
  EPI_PATCH = 4,       // C(f32)[img*(np+1)+1+p, n] = acc + pos[(1+p), n]   (m = img*np + p)
  // LayerNorm folded into the GEMMs on either side of it (16-bit engines; modeling_clip.py:370-381: LN -> Linear):
  //   the Linear's weights carry LayerNorm's gain AND its centring (W' = W * g with each row's mean over k removed, so
  //   x . W'^T == (x - mean(x)) . (W * g)^T: the mean subtraction happens inside the contraction), its bias carries
  //   LayerNorm's bias (c2 = W b + bias), the A operand is the bf16 residual stream itself, and only the row's rstd
  //   enters in the epilogue:   y = rstd[m] * acc + c2[n]
  EPI_BIAS_LN = 5,     // C(bf16) = that                                   (LN1 -> q/k/v)
  EPI_QGELU_LN = 6,    // C(bf16) = quickgelu(that)                        (LN2 -> fc1)
  // ... and the producer of the NEXT LayerNorm's input: the in-place residual update also emits the bf16 copy of the
  // new rows (the next GEMM's A operand) and their statistics as per-64-column partials {sum, centred M2}
  EPI_RESID_EMIT = 7,  // C(f32) += acc + bias[n];  xb(bf16) = C;  st[m, n/64] = {sum, M2}
  // The same update on a residual stream kept as TWO planes (common.h split_f32): hi = the fp32 value rounded to the operand type, lo =
  // an 8-bit remainder -- the stream at 16 (bf16) / 19 (f16) significand bits, its hi plane IS the next GEMM's A operand, and the
  // epilogue moves 6 bytes per element (3 in, 3 out) instead of the 10 of EPI_RESID_EMIT (which writes fp32 and a separate 16-bit copy).
  EPI_RESID_SPLIT = 8, // {hi,lo} += acc + bias[n] (xb_out = hi, lo_io = lo);  st[m, n/64] = {sum, M2}
  // The exact (erf) GELU of hidden_act = "gelu" towers (common.h erf_gelu), appended so that the numbers above keep their values:
  EPI_BIAS_GELU = 9,   // C(T)   = gelu(acc + bias[n])
  EPI_GELU_LN = 10,    // C(bf16) = gelu(rstd[m] * acc + c2[n])            (LN2 -> fc1)
  EPI_COUNT = 11
};
constexpr bool epi_is_ln(int e) { return e == EPI_BIAS_LN || e == EPI_QGELU_LN || e == EPI_GELU_LN; }
constexpr bool epi_is_colwise(int e) { return e == EPI_BIAS || e == EPI_BIAS_QGELU || e == EPI_BIAS_GELU || epi_is_ln(e); }
constexpr bool epi_is_resid(int e) { return e == EPI_BIAS_RESID || e == EPI_RESID_EMIT || e == EPI_RESID_SPLIT; }
constexpr bool epi_emits_stats(int e) { return e == EPI_RESID_EMIT || e == EPI_RESID_SPLIT; }

struct GemmParams {
  const void* A;
  const void* W;
  void* C;
  const float* bias;  // [N] (EPI_BIAS*) or position embedding [(np+1), N] (EPI_PATCH)
  int M, N, K;
  int lda, ldw, ldc;  // in elements
  float alpha;
  int np;             // patches per image (EPI_PATCH)
  // EPI_*_LN consumers: per-row statistics partials [M, ln_ns, 2] fp32 over 64-column slices of the LayerNorm input
  // (ln_combine; bias carries c2), 1/D and eps of that LayerNorm
  const float* ln_stats = nullptr;
  int ln_ns = 0;
  float ln_inv_d = 0.f, ln_eps = 0.f;
  // EPI_RESID_EMIT producer: bf16 copy of the updated rows [M, ldc] and their partial statistics [M, N/64, 2].
  // EPI_RESID_SPLIT: xb_out is the hi plane (16-bit, read AND written), lo_io the lo plane (8-bit, blocked layout, read and written)
  void* xb_out = nullptr;
  float* st_out = nullptr;
  void* lo_io = nullptr;
  // EPI_RESID_SPLIT: write the updated planes in the OTHER 16-bit type's split format (read them in T's): the last f16 block
  // of a mixed text tower (plipmi_config.text_f16_layers) hands the stream to the bf16 blocks without a re-coding pass.
  // (The epilogue splits the value it computed in fp32: no double rounding through T's format.)
  int planes_other = 0;
  // ADDR 2 (the patch GEMM, im2col ON LOAD; modeling_clip.py:148-154,209-210): A is not read as [M, K] rows -- row m = patch (img, gi, gj)
  // and column k = (c, u, v) are GATHERED from the fp32 NCHW pixels while a K tile is staged: four consecutive pixels of one image row
  // per lane into registers, rounded to the operand type, written to the A stage (LDS-DMA copies bytes, it cannot convert: this is the
  // register-staged converting A path).  pix = the pixels, img_h x img_w = image rows x columns (row stride img_w, plane stride
  // img_h * img_w; the patch grid is (img_h >> patch_log2) x (img_w >> patch_log2), pixels past it are never read -- HF's strided conv
  // floors the same way), patch_log2 = log2 of the patch side (4 or 5).
  const float* pix = nullptr;
  int img_h = 0, img_w = 0, patch_log2 = 0;
  // ADDR 3: the same gather from native uint8 HWC tiles [B, H, W, 3] (plipmi_encode_image_u8; reproducibility/embedders/transform.py:45-52
  // on 224 x 224 tiles reduces to (u8 / 255 - mean) / std): a lane loads the 12 bytes of four RGB pixels, takes the K tile's channel and
  // normalises with ONE fma per pixel -- fl(b * A_c + B_c) rounds to the same bf16 / f16 as the unfold kernel's (b / 255 - mean_c) * (1 / std_c)
  // for every byte value and channel (exhaustive: tests/test_host.py::test_u8_normalisation_by_one_fma_is_exact_after_rounding)
  const unsigned char* tiles = nullptr;
  // Row count known only on the device (packed captions, kernels.h launch_text_pack): when set, the kernel processes
  // min(*m_dev, M) rows -- M then only sizes the grid; workgroups whose tile starts past the live rows exit at once
  const int* m_dev = nullptr;
  // Tile raster: the N tiles are cut in column groups `gw` tiles wide; logical tile ids run group by group,
  // M-major inside a group.  An XCD's contiguous id range is then a compact (rows x gw) patch whose W panels
  // (gw*BN rows of W) stay resident in its 4 MiB L2 while the A row panels stream through once.
  // 0 = one group (N-major sweep of whole rows).  Set by gemm_launch.
  int gw = 0;
  // test hook (plipmi_gemm_nt_traced): per workgroup 8 x u64 {start, prologue done, main loop done, epilogue
  // done, logical tile id, HW_ID, k tiles, 0}, s_memtime ticks.  nullptr on the product path.
  unsigned long long* trace = nullptr;
};

// ---- host side ----------------------------------------------------------------
struct GemmVariant {
  const char* name;
  int bm, bn, threads;
};
int gemm_num_variants();
int gemm_num_cus();   // compute units of the current device, rounded down to a multiple of 8 (gemm.hip)
const GemmVariant& gemm_variant(int v);
// dtype: 0 fp32, 1 bf16, 2 f16.  variant -1 = auto, -2 = naive.  Returns hipError_t as int; *kernel_name (optional)
// receives a static string naming the kernel that ran.
// (variant -1: the tile with the smallest rounds x tile-time on this shape, gemm.hip)
int gemm_launch(int dtype, int epi, int variant, const GemmParams& p, hipStream_t stream, const char** kernel_name);
int gemm_default_variant(int dtype, int M, int N, int K);
bool gemm_variant_is_built(int dtype, int variant);
// small-M kernel of the 16-bit engines (gemm_skinny.hip): 32 x 64 output tile per workgroup, K split over its waves
bool gemm_skinny_supports(int epi, int M, int N, int K);
int gemm_launch_skinny(int dtype, int epi, const GemmParams& p, hipStream_t stream, const char** kernel_name);
// tests / A-B runs (process-wide hooks behind plipmi_test.h, not product knobs); false = value out of range, nothing changed
bool gemm_force_tile(int variant);            // -1 the cost model chooses, -2 the naive checker, >= 0 that tile for every launch
bool gemm_remap_tile(int from, int to);       // the cost model's choice `from` runs as tile `to` (-1: as itself again)
void gemm_reset_overrides();
// the patch GEMM with its A operand gathered from fp32 pixels while it is staged (ADDR 2: im2col on load, no unfold pass)
bool gemm_gather_supports(int dtype, int B, int img_h, int img_w, int patch, int N);
int gemm_launch_gather(int dtype, const GemmParams& p, hipStream_t stream, const char** kernel_name);

}  // namespace plipmi

