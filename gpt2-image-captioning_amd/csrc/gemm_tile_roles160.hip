#include "gemm_launch.h"

namespace icap {

// Variant 32 (round 6): 160 x 128 tiles on the split-role ring (gemm_tile.h ROLES): 4 MFMA waves of 80 x 64 + 4 LDS-DMA
// waves, 4 stages of 36 KiB (two in flight), one block per CU. For the N <= 1024 products of more rows than one round of
// 96 x 128 tiles holds: CLIP-B/32's 6400 x 768 out_proj / fc2 are 40 x 6 = 240 tiles (96 x 128: 402, 1.6 rounds).
int launch_tile_roles160(const GemmPlan& pl, const icap_gemm_args& p, int nks, hipStream_t s) {
  return launch_tile_forms<bf16_t, KINDS_ALL, V_ROLES160>(pl, p, nks, s);
}

}  // namespace icap
