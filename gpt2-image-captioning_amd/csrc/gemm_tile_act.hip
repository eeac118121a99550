#include "gemm_launch.h"

namespace icap {

// Activation-specialised epilogues of the 128-row tiles (the fwd / bwd columns of gemm_plan.h TILE_VARIANTS; bf16 in /
// out): gelu_new on variants 0 / 4 / 5 (0: GPT-2 large / medium c_fc, K = 1280 / 1024 > 16 stages), quick_gelu and erf
// gelu on 4, relu on 13
int launch_tile_act(const GemmPlan& pl, const icap_gemm_args& p, int nks, hipStream_t s) {
  return launch_tile_forms<bf16_t, KINDS_ACT, V_DB, V_S3, V_S4, V_N13>(pl, p, nks, s);
}

}  // namespace icap
