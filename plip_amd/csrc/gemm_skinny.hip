// gemm_skinny.hip -- the NT GEMM for SMALL M (latency regime):  C = epilogue(A[M,K] . W[N,K]^T), 16-bit operands (bf16 / f16).
//
// Where the big-tile kernel (gemm.h) walks K one 64-deep tile after the other on a handful of workgroups -- M = 256
// rows x N = 768 is 12 workgroups of 128x128, each 48 dependent K iterations for fc2 = 35-55 us -- this kernel spends
// the chip's width on N, on M and on K at once:
//   * one workgroup (NW = 4 or 8 waves) owns a 32 x 64 output tile and its waves split K NW ways (fixed-order reduction
//     through LDS: deterministic, independent of M); a wave requests NB 64-deep blocks of both operands (all of its share
//     when that is <= 3 blocks) before the first MFMA, so its K walk is 1-3 memory round trips, not one per block;
//   * operands come straight from L2 as MFMA fragments -- no LDS staging, nothing to synchronise in the K loop.  The k
//     index inside an MFMA may be permuted freely as long as both operands share the permutation, so a lane fetches 64
//     CONTIGUOUS bytes of its row per 64-deep block (lanes l and l+32 together one whole 128-byte line) and feeds
//     MFMA t of the block from the t-th 16-byte piece;
//   * the same fused epilogues as the big kernel's LayerNorm-folded family: rstd * acc + c2 (-> bf16, optional
//     QuickGELU), and the in-place fp32 residual update that also emits bf16(x) and the row's {sum, centred M2} of the
//     64-column slice (= exactly this tile's width).
// Used by the 16-bit engines (a) for the LAST block of each tower, whose out_proj / fc1 / fc2 only ever matter for the pooled
// row of each sample (engine.hip: run_last_block_pooled): M = batch size, at every batch size; and (b), round 4, for EVERY GEMM
// of a small batch (engine.hip: latency path, batches of at most plipmi_engine::latency_batch samples -- the reference drives
// its heads at batch 8, plip.py:90-91): the big tiles walk K serially whatever M is (fc2: 48 dependent K tiles = 45 us for
// 400 rows), this kernel splits it 8 ways.  A row's result never depends on the other rows of ITS call, so embeddings are
// bit-identical across batch sizes within each of the two regimes; between them they differ by fp32 summation order.
#include "gemm_skinny_kernel.h"

namespace plipmi {

bool gemm_skinny_supports(int epi, int M, int N, int K) {
  const bool epi_ok = epi == EPI_BIAS || epi == EPI_BIAS_QGELU || epi == EPI_BIAS_RESID || epi == EPI_BIAS_LN ||
                      epi == EPI_QGELU_LN || epi == EPI_RESID_EMIT || epi == EPI_RESID_SPLIT || epi == EPI_PATCH ||
                      epi == EPI_BIAS_GELU || epi == EPI_GELU_LN;
  return epi_ok && M > 0 && N % SK_BN == 0 && K % 256 == 0;
}

template <typename T>
static int launch_skinny_epi(int epi, const GemmParams& p, hipStream_t s) {
  switch (epi) {
    case EPI_BIAS: return launch_skinny<T, EPI_BIAS>(p, s);
    case EPI_BIAS_QGELU: return launch_skinny<T, EPI_BIAS_QGELU>(p, s);
    case EPI_BIAS_RESID: return launch_skinny<T, EPI_BIAS_RESID>(p, s);
    case EPI_BIAS_LN: return launch_skinny<T, EPI_BIAS_LN>(p, s);
    case EPI_QGELU_LN: return launch_skinny<T, EPI_QGELU_LN>(p, s);
    case EPI_RESID_EMIT: return launch_skinny<T, EPI_RESID_EMIT>(p, s);
    case EPI_RESID_SPLIT: return launch_skinny<T, EPI_RESID_SPLIT>(p, s);
    case EPI_PATCH: return launch_skinny<T, EPI_PATCH>(p, s);
    default: return (int)hipErrorInvalidValue;
  }
}

int gemm_launch_skinny(int dtype, int epi, const GemmParams& p, hipStream_t s, const char** kernel_name) {
  if (p.M <= 0) return 0;
  if ((dtype != 1 && dtype != 2) || !gemm_skinny_supports(epi, p.M, p.N, p.K) || p.lda % 8 || p.ldw % 8) return (int)hipErrorInvalidValue;
  static const char* names[2][EPI_COUNT] = {
      {"gemm_skinny<bf16,32x64_splitk,bias>", "gemm_skinny<bf16,32x64_splitk,bias_qgelu>", "gemm_skinny<bf16,32x64_splitk,bias_resid>",
       nullptr, "gemm_skinny<bf16,32x64_splitk,patch>", "gemm_skinny<bf16,32x64_splitk,ln_bias>", "gemm_skinny<bf16,32x64_splitk,ln_qgelu>",
       "gemm_skinny<bf16,32x64_splitk,resid_emit>", "gemm_skinny<bf16,32x64_splitk,resid_split>",
       "gemm_skinny<bf16,32x64_splitk,bias_gelu>", "gemm_skinny<bf16,32x64_splitk,ln_gelu>"},
      {"gemm_skinny<f16,32x64_splitk,bias>", "gemm_skinny<f16,32x64_splitk,bias_qgelu>", "gemm_skinny<f16,32x64_splitk,bias_resid>",
       nullptr, "gemm_skinny<f16,32x64_splitk,patch>", "gemm_skinny<f16,32x64_splitk,ln_bias>", "gemm_skinny<f16,32x64_splitk,ln_qgelu>",
       "gemm_skinny<f16,32x64_splitk,resid_emit>", "gemm_skinny<f16,32x64_splitk,resid_split>",
       "gemm_skinny<f16,32x64_splitk,bias_gelu>", "gemm_skinny<f16,32x64_splitk,ln_gelu>"}};
  if (kernel_name) *kernel_name = names[dtype - 1][epi];
  if (epi == EPI_BIAS_GELU || epi == EPI_GELU_LN) return gemm_launch_skinny_gelu(dtype, epi, p, s);
  return with_half(dtype, [&](auto tag) { return launch_skinny_epi<decltype(tag)>(epi, p, s); });
}

}  // namespace plipmi
