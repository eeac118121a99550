#include "gemm_tile.h"
#include "gemm_launch.h"

namespace icap {

// The LayerNorm statistics hand-off forms (bf16 in / out; gemm_plan.cpp tile128_caps lists the combinations): producers
// (ACT_LNS, no activation) and consumers (ACT_LNF: no activation, gelu_new, quick_gelu; 128 x 64 tiles with the
// dispatching form)
int launch_tile_ln(const GemmPlan& pl, const icap_gemm_args& p, int nks, hipStream_t s) {
  ICAP_TILE_PRELUDE;
#define ICAP_GKL(NST, MINB, TM_, TN_, KIND) \
  hipLaunchKernelGGL((gemm_kernel<bf16_t, bf16_t, NST, MINB, 2, 2, TM_, TN_, false, KIND>), grid, block, 0, s, p, tn, sp, \
                     nks, thr, inv_keep)
#define ICAP_GKL_V(KIND)                                     \
  switch (pl.variant) {                                      \
    case V_DB: ICAP_GKL(2, 2, 4, 4, KIND); break;            \
    case V_S3: ICAP_GKL(1, 3, 4, 4, KIND); break;            \
    case V_S4: ICAP_GKL(1, 4, 4, 4, KIND); break;            \
    case V_N12: ICAP_GKL(2, 3, 4, 2, KIND); break;           \
    case V_N13: ICAP_GKL(1, 4, 4, 2, KIND); break;           \
    default: return gemm_no_instantiation(pl);               \
  }
  switch (pl.actk) {
    case ACT_LNS + ACT_OFF: ICAP_GKL_V(ACT_LNS + ACT_OFF) break;
    case ACT_LNF + ACT_OFF: ICAP_GKL_V(ACT_LNF + ACT_OFF) break;
    case ACT_LNF + ACT_FWD + ICAP_ACT_GELU_NEW:
      if (pl.variant == V_DB) ICAP_GKL(2, 2, 4, 4, ACT_LNF + ACT_FWD + ICAP_ACT_GELU_NEW);
      else if (pl.variant == V_S3) ICAP_GKL(1, 3, 4, 4, ACT_LNF + ACT_FWD + ICAP_ACT_GELU_NEW);
      else if (pl.variant == V_S4) ICAP_GKL(1, 4, 4, 4, ACT_LNF + ACT_FWD + ICAP_ACT_GELU_NEW);
      else return gemm_no_instantiation(pl);
      break;
    case ACT_LNF + ACT_FWD + ICAP_ACT_QUICK_GELU:
      if (pl.variant != V_S3) return gemm_no_instantiation(pl);
      ICAP_GKL(1, 3, 4, 4, ACT_LNF + ACT_FWD + ICAP_ACT_QUICK_GELU);
      break;
    case ACT_LNF + ACT_ANY:  // 128 x 64
      if (pl.variant == V_N12) ICAP_GKL(2, 3, 4, 2, ACT_LNF + ACT_ANY);
      else if (pl.variant == V_N13) ICAP_GKL(1, 4, 4, 2, ACT_LNF + ACT_ANY);
      else return gemm_no_instantiation(pl);
      break;
    default: return gemm_no_instantiation(pl);
  }
#undef ICAP_GKL_V
#undef ICAP_GKL
  return ICAP_OK;
}

}  // namespace icap
