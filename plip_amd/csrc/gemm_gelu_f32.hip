// fp32 (v_mfma_f32_32x32x2_f32; the activation with the device library's erff) instantiations of the NT GEMM's exact-GELU epilogues (gemm.h EPI_BIAS_GELU / EPI_GELU_LN: the fc1 GEMM of a
// hidden_act = "gelu" tower), in a unit of their own: gemm_f32.hip's code object is the same with and without them.
#include "gemm_inst.h"
namespace plipmi {
GemmLaunchFn gemm_get_gelu_f32(int variant, int epi) { return gemm_gelu_pick<float>(variant, epi); }
}  // namespace plipmi
