#include "gemm_tile.h"
#include "gemm_launch.h"

namespace icap {

// K-outer operands (trans_ab; bf16 inputs): double-buffered (14) / single-stage (15)
int launch_tile_kout(const GemmPlan& pl, const icap_gemm_args& p, int nks, hipStream_t s) {
  ICAP_TILE_PRELUDE;
  if (pl.variant != V_KOUT_DB && pl.variant != V_KOUT_S3) return gemm_no_instantiation(pl);
  if (p.c_dtype == ICAP_BF16) {
    if (pl.variant == V_KOUT_DB) ICAP_GK(bf16_t, bf16_t, 2, 2, 4, 4, true);
    else ICAP_GK(bf16_t, bf16_t, 1, 3, 4, 4, true);
  } else {
    if (pl.variant == V_KOUT_DB) ICAP_GK(bf16_t, float, 2, 2, 4, 4, true);
    else ICAP_GK(bf16_t, float, 1, 3, 4, 4, true);
  }
  return ICAP_OK;
}

}  // namespace icap
