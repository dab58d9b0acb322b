// gemm_skinny_gelu.hip -- the exact-GELU epilogues (gemm.h EPI_BIAS_GELU / EPI_GELU_LN) of the small-M split-K kernel, in a unit of
// their own: gemm_skinny.hip's code object is the same with and without them.
#include "gemm_skinny_kernel.h"

namespace plipmi {

int gemm_launch_skinny_gelu(int dtype, int epi, const GemmParams& p, hipStream_t s) {
  return with_half(dtype, [&](auto tag) {
    using T = decltype(tag);
    return epi == EPI_BIAS_GELU ? launch_skinny<T, EPI_BIAS_GELU>(p, s) : launch_skinny<T, EPI_GELU_LN>(p, s);
  });
}

}  // namespace plipmi
