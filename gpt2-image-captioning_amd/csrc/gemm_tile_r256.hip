#include "gemm_launch.h"

namespace icap {

// Variant 22: 256 x 128 tiles of 8 waves (4 x 2, 64 x 64 each) on the 3-stage LDS-DMA ring, one block per CU
// (gemm_tile.h, NST >= 3), bf16 inputs, every epilogue form the plan may give it (round 5).
int launch_tile_r256(const GemmPlan& pl, const icap_gemm_args& p, int nks, hipStream_t s) {
  return launch_tile_forms<bf16_t, KINDS_ALL, V_R256>(pl, p, nks, s);
}

}  // namespace icap
