#include "gemm_launch.h"

namespace icap {

// Variant 24: 192 x 64 tiles of 4 waves stacked in M (4 x 1, 48 x 64 each), double-buffered LDS-DMA at 2 blocks per
// CU (gemm_tile.h, NST 2), bf16 inputs (round 5). For the N = 768 products of the packed step: 3584 x 768 is 19 x 12
// = 228 tiles, one round over 256 CUs, where 128 x 64 tiles make 336 (1.3 rounds) and 128 x 128 make 168 (two thirds
// of the CUs). hipBLASLt runs those shapes on one round of 128 x 96 tiles (profiles/r05_blaslt_kernels.txt); 96
// columns per tile do not split into the 32-column groups of the LayerNorm statistics epilogue, 64 do.
// Variant 25: the same tiles on the LDS-DMA ring (gemm_tile.h NST 4: three stages in flight, one
// block per CU) for long K. (Round 5 also measured a fragment prefetch across the ring's stages and a register-staged
// double buffer on these tiles — bitwise equal, neither faster: profiles/r05_w192_ab.txt; removed.)
int launch_tile_w192(const GemmPlan& pl, const icap_gemm_args& p, int nks, hipStream_t s) {
  return launch_tile_forms<bf16_t, KINDS_ALL, V_W192, V_W192_RING>(pl, p, nks, s);
}

}  // namespace icap
