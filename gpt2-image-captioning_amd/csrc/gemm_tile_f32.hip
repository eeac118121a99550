#include "gemm_launch.h"

namespace icap {

// fp32 inputs (the parity mode: exact-fp32 16x16x4 MFMA chains): variants 0 / 4 / 5
int launch_tile_f32(const GemmPlan& pl, const icap_gemm_args& p, int nks, hipStream_t s) {
  return launch_tile_forms<float, KINDS_ALL, V_DB, V_S3, V_S4>(pl, p, nks, s);
}

}  // namespace icap
