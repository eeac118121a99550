#include "gemm_launch.h"

namespace icap {

// MX block-scaled fp8 inputs: variants 0 / 4 only (gemm_plan.h TILE_VARIANTS)
int launch_tile_mx(const GemmPlan& pl, const icap_gemm_args& p, int nks, hipStream_t s) {
  return launch_tile_forms<fp8_t, KINDS_ALL, V_DB, V_S3>(pl, p, nks, s);
}

}  // namespace icap
