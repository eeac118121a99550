#include "gemm_launch.h"

namespace icap {

// The LayerNorm statistics hand-off forms (bf16 in / out; gemm_plan.h TILE_VARIANTS lists the combinations): producers
// (ACT_LNS, no activation) and consumers (ACT_LNF: no activation, gelu_new, quick_gelu; 128 x 64 tiles with the
// dispatching form)
int launch_tile_ln(const GemmPlan& pl, const icap_gemm_args& p, int nks, hipStream_t s) {
  return launch_tile_forms<bf16_t, KINDS_LN, V_DB, V_S3, V_S4, V_N12, V_N13>(pl, p, nks, s);
}

}  // namespace icap
