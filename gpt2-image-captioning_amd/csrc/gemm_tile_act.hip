#include "gemm_tile.h"
#include "gemm_launch.h"

namespace icap {

// Activation-specialised epilogues (gemm_plan.cpp tile128_caps: bf16 in / out, variants 0, 4, 5, 13)
int launch_tile_act(const GemmPlan& pl, const icap_gemm_args& p, int nks, hipStream_t s) {
  ICAP_TILE_PRELUDE;
#define ICAP_GKS(NST, MINB, TM_, TN_, KIND) \
  hipLaunchKernelGGL((gemm_kernel<bf16_t, bf16_t, NST, MINB, 2, 2, TM_, TN_, false, KIND>), grid, block, 0, s, p, tn, sp, \
                     nks, thr, inv_keep)
#define ICAP_GKS_V045(KIND)                                  \
  switch (pl.variant) {                                      \
    case V_DB: ICAP_GKS(2, 2, 4, 4, KIND); break;            \
    case V_S3: ICAP_GKS(1, 3, 4, 4, KIND); break;            \
    case V_S4: ICAP_GKS(1, 4, 4, 4, KIND); break;            \
    default: return gemm_no_instantiation(pl);               \
  }
  const int v = pl.variant;
  switch (pl.actk) {
    // (variant 0: GPT-2 large / medium c_fc, K = 1280 / 1024 > 16 stages)
    case ACT_FWD + ICAP_ACT_GELU_NEW: ICAP_GKS_V045(ACT_FWD + ICAP_ACT_GELU_NEW) break;
    case ACT_BWD + ICAP_ACT_GELU_NEW: ICAP_GKS_V045(ACT_BWD + ICAP_ACT_GELU_NEW) break;
    case ACT_FWD + ICAP_ACT_QUICK_GELU:
      if (v != V_S3) return gemm_no_instantiation(pl);
      ICAP_GKS(1, 3, 4, 4, ACT_FWD + ICAP_ACT_QUICK_GELU);
      break;
    case ACT_FWD + ICAP_ACT_GELU_ERF:
      if (v != V_S3) return gemm_no_instantiation(pl);
      ICAP_GKS(1, 3, 4, 4, ACT_FWD + ICAP_ACT_GELU_ERF);
      break;
    case ACT_FWD + ICAP_ACT_RELU:
      if (v != V_N13) return gemm_no_instantiation(pl);
      ICAP_GKS(1, 4, 4, 2, ACT_FWD + ICAP_ACT_RELU);
      break;
    case ACT_BWD + ICAP_ACT_RELU:
      if (v != V_N13) return gemm_no_instantiation(pl);
      ICAP_GKS(1, 4, 4, 2, ACT_BWD + ICAP_ACT_RELU);
      break;
    default: return gemm_no_instantiation(pl);
  }
#undef ICAP_GKS_V045
#undef ICAP_GKS
  return ICAP_OK;
}

}  // namespace icap
