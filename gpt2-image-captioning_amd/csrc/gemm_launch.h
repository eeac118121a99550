// The per-form launchers of the tile kernel (gemm_tile_*.hip: one translation unit per input form, so their
// instantiations compile in parallel) and the helpers they are written with.
#pragma once
#include "gemm_common.h"
#include "gemm_plan.h"

namespace icap {
// Launch the tile-kernel instantiation pl selects (grid pl.grid_x, block pl.block_x); nks = nk_split | skew / diag
// bits. ICAP_ERR_ARG (gemm_no_instantiation) for a (variant, epilogue kind) the unit does not instantiate.
int launch_tile_bf16(const GemmPlan& pl, const icap_gemm_args& p, int nks, hipStream_t s);  // variants 0/4/5/12/13/16
int launch_tile_act(const GemmPlan& pl, const icap_gemm_args& p, int nks, hipStream_t s);   // specialised epilogues
int launch_tile_kout(const GemmPlan& pl, const icap_gemm_args& p, int nks, hipStream_t s);  // K-outer (14 / 15)
int launch_tile_mx(const GemmPlan& pl, const icap_gemm_args& p, int nks, hipStream_t s);    // MX fp8 (0 / 4)
int launch_tile_f32(const GemmPlan& pl, const icap_gemm_args& p, int nks, hipStream_t s);   // fp32 parity (0 / 4 / 5)
int launch_tile_ln(const GemmPlan& pl, const icap_gemm_args& p, int nks, hipStream_t s);    // LN statistics hand-off
int launch_tile_r256(const GemmPlan& pl, const icap_gemm_args& p, int nks, hipStream_t s);  // 256 x 128 ring (22)
int launch_tile_w192(const GemmPlan& pl, const icap_gemm_args& p, int nks, hipStream_t s);  // 192 x 64 (24)
int launch_tile_roles(const GemmPlan& pl, const icap_gemm_args& p, int nks, hipStream_t s);    // roles 128 x 256 (26)
int launch_tile_roles96(const GemmPlan& pl, const icap_gemm_args& p, int nks, hipStream_t s);  // roles 96 x 128 (27)
int launch_tile_roles192(const GemmPlan& pl, const icap_gemm_args& p, int nks, hipStream_t s); // roles 192 x 256 (28)
int launch_tile_roles_kout(const GemmPlan& pl, const icap_gemm_args& p, int nks, hipStream_t s); // roles K-outer (31)
int launch_tile_roles160(const GemmPlan& pl, const icap_gemm_args& p, int nks, hipStream_t s);  // roles 160 x 128 (32)
// a group of K-outer weight-gradient products run in one launch (icap_gemm_group)
constexpr int ICAP_GEMM_GROUP_MAX = 8;
struct GemmGroup {
  icap_gemm_args a[ICAP_GEMM_GROUP_MAX];
  int tiles_n[ICAP_GEMM_GROUP_MAX];
  int nk[ICAP_GEMM_GROUP_MAX];
  int tstart[ICAP_GEMM_GROUP_MAX + 1];
  int n;
};
void launch_group_kout(const GemmGroup& g, int cus, hipStream_t s);

}  // namespace icap

// The launch helpers of the gemm_tile_*.hip units (each defines its launcher with these).
#define ICAP_TILE_PRELUDE                                       \
  const dim3 grid(pl.grid_x, pl.grid_y), block(pl.block_x);     \
  const int sp = pl.splits, tn = pl.tiles_n;                    \
  const uint32_t thr = pl.thr;                                  \
  const float inv_keep = pl.inv_keep
#define ICAP_GK(TI, TC, NST, MINB, TM_, TN_, KOUT)                                                              \
  do {                                                                                                       \
    if (pl.actk == ACT_ANY) hipLaunchKernelGGL((gemm_kernel<TI, TC, NST, MINB, 2, 2, TM_, TN_, KOUT, ACT_ANY>), grid, block, 0, s, p, tn, sp, nks, thr, inv_keep); \
    else if (pl.actk == ACT_OFF) hipLaunchKernelGGL((gemm_kernel<TI, TC, NST, MINB, 2, 2, TM_, TN_, KOUT, ACT_OFF>), grid, block, 0, s, p, tn, sp, nks, thr, inv_keep); \
    else return gemm_no_instantiation(pl);                                                                     \
  } while (0)
#define ICAP_GEMM_LAUNCH(TI, TC)                                    \
  switch (pl.variant) {                                             \
    case V_DB: ICAP_GK(TI, TC, 2, 2, 4, 4, false); break;           \
    case V_S3: ICAP_GK(TI, TC, 1, 3, 4, 4, false); break;           \
    case V_S4: ICAP_GK(TI, TC, 1, 4, 4, 4, false); break;           \
    default: return gemm_no_instantiation(pl);                      \
  }
