#include "gemm_launch.h"

namespace icap {

// Variant 27 (round 6): 96 x 128 tiles on the split-role ring (gemm_tile.h ROLES): 4 MFMA waves of 48 x 64 + 4 LDS-DMA
// waves, 5 stages of 28 KiB (three in flight), one block per CU. For the N <= 1024 products: 3584 x 768 is 38 x 6 = 228
// tiles, one round over 256 CUs with no split of K (GPT-2's N = 768 products at K = 768 / 2304 / 3072).
int launch_tile_roles96(const GemmPlan& pl, const icap_gemm_args& p, int nks, hipStream_t s) {
  return launch_tile_forms<bf16_t, KINDS_ALL, V_ROLES96>(pl, p, nks, s);
}

}  // namespace icap
