#include "gemm_launch.h"

namespace icap {

// Variant 26 (round 6): 128 x 256 tiles, the split-role ring of gemm_tile.h (ROLES): 4 MFMA waves of 64 x 128 (one per
// SIMD) + 4 LDS-DMA waves, 3 stages of 48 KiB, one block per CU. For the products with N >= 2048 whose 128 x 256 tiles
// fill about one round (GPT-2's 3584 x 2304 x 768 c_attn: 252 tiles). Every epilogue form the plan may give it.
int launch_tile_roles(const GemmPlan& pl, const icap_gemm_args& p, int nks, hipStream_t s) {
  return launch_tile_forms<bf16_t, KINDS_ALL, V_ROLES>(pl, p, nks, s);
}

}  // namespace icap
