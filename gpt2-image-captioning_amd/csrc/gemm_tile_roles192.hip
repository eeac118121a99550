#include "gemm_launch.h"

namespace icap {

// Variant 28 (round 6): 192 x 256 tiles on the split-role ring (gemm_tile.h ROLES) with 8 MFMA waves (2 x 4, 96 x 64
// each, two per SIMD) + 4 LDS-DMA waves, 2 stages of 56 KiB, one block per CU: for the N = 3072 products of the step
// (3584 x 3072 is 19 x 12 = 228 tiles, one round; 128 x 256 tiles make 336, two rounds).
int launch_tile_roles192(const GemmPlan& pl, const icap_gemm_args& p, int nks, hipStream_t s) {
  return launch_tile_forms<bf16_t, KINDS_ALL, V_ROLES192>(pl, p, nks, s);
}

}  // namespace icap
