#include "gemm_launch.h"

namespace icap {

// K-outer operands (trans_ab; bf16 inputs): double-buffered (14) / single-stage (15)
int launch_tile_kout(const GemmPlan& pl, const icap_gemm_args& p, int nks, hipStream_t s) {
  return launch_tile_forms<bf16_t, KINDS_ALL, V_KOUT_DB, V_KOUT_S3>(pl, p, nks, s);
}

}  // namespace icap
