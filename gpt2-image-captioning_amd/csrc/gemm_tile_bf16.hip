#include "gemm_launch.h"

namespace icap {

// bf16 inputs, runtime-dispatch (ACT_ANY) or activation-free (ACT_OFF) epilogues: 128 x 128 (variants 0 / 4 / 5),
// the 4-stage ring (16), 128 x 64 (12 / 13)
int launch_tile_bf16(const GemmPlan& pl, const icap_gemm_args& p, int nks, hipStream_t s) {
  return launch_tile_forms<bf16_t, KINDS_PLAIN, V_DB, V_S3, V_S4, V_N12, V_N13, V_RING>(pl, p, nks, s);
}

}  // namespace icap
