// The launch plan icap_gemm makes for one call, and the host-only planner that makes it (gemm_plan.cpp). No HIP
// dependency: the planner never dereferences an operand pointer, so a host compiler can exercise it without a GPU
// (plan_check.cpp).
#pragma once
#include "gemm_consts.h"
#include "host_common.h"

namespace icap {

// The instantiations of the tile kernel (gemm_tile.h gemm_kernel<TI, TC, NST, MINB, WM, WN, TM, TN, KOUT, ACT, ROLES>),
// one row each. The ids are the numbers DESIGN.md, profiles/ and the tests use.
enum TileVariant : int {
  V_DB = 0,            // 128 x 128, double-buffered, 2 blocks / CU
  V_S3 = 4,            // 128 x 128, single LDS buffer, 3 blocks / CU
  V_S4 = 5,            // 128 x 128, single LDS buffer, 4 blocks / CU
  V_N12 = 12,          // 128 x 64, double-buffered, 3 blocks / CU
  V_N13 = 13,          // 128 x 64, single LDS buffer, 4 blocks / CU
  V_KOUT_DB = 14,      // K-outer operands (trans_ab): form of 0
  V_KOUT_S3 = 15,      // K-outer operands: form of 4
  V_RING = 16,         // 128 x 128 on the 4-stage ring, 1 block / CU
  V_R256 = 22,         // 256 x 128, 8 waves, 3-stage ring
  V_W192 = 24,         // 192 x 64, 4 waves stacked in M, double-buffered
  V_W192_RING = 25,    // 192 x 64 on the 4-stage ring
  V_ROLES = 26,        // split-role ring (MFMA waves + 4 LDS-DMA waves), 128 x 256
  V_ROLES96 = 27,      // split-role ring, 96 x 128
  V_ROLES192 = 28,     // split-role ring, 8 MFMA waves, 192 x 256
  V_ROLES_KOUT = 31,   // split-role ring, K-outer operands, 128 x 128
  V_ROLES160 = 32,     // split-role ring, 160 x 128
};
struct TileVariantInfo {
  int id, nst, minb, wm, wn, tm, tn;
  bool kout, roles;
  constexpr int bm() const { return wm * tm * 16; }                          // tile rows
  constexpr int bn() const { return wn * tn * 16; }                          // tile columns
  constexpr int threads() const { return (wm * wn + (roles ? 4 : 0)) * 64; }  // (+ the 4 LDS-DMA waves)
  // the split-role variants walk K in its natural order (one round of tiles, no lockstep panel misses to stagger,
  // and automatic launches then equal forced ones and the tile path bitwise); the others take the K-skew
  constexpr bool natural_k() const { return roles; }
};
constexpr TileVariantInfo TILE_VARIANTS[] = {
    // id            NST MINB WM WN TM TN KOUT   ROLES
    {V_DB,           2,  2,   2, 2, 4, 4, false, false},
    {V_S3,           1,  3,   2, 2, 4, 4, false, false},
    {V_S4,           1,  4,   2, 2, 4, 4, false, false},
    {V_N12,          2,  3,   2, 2, 4, 2, false, false},
    {V_N13,          1,  4,   2, 2, 4, 2, false, false},
    {V_KOUT_DB,      2,  2,   2, 2, 4, 4, true,  false},
    {V_KOUT_S3,      1,  3,   2, 2, 4, 4, true,  false},
    {V_RING,         4,  1,   2, 2, 4, 4, false, false},
    {V_R256,         3,  1,   4, 2, 4, 4, false, false},
    {V_W192,         2,  2,   4, 1, 3, 4, false, false},
    {V_W192_RING,    4,  1,   4, 1, 3, 4, false, false},
    {V_ROLES,        3,  1,   2, 2, 4, 8, false, true},
    {V_ROLES96,      5,  1,   2, 2, 3, 4, false, true},
    {V_ROLES192,     2,  1,   2, 4, 6, 4, false, true},
    {V_ROLES_KOUT,   4,  1,   2, 2, 4, 4, true,  true},
    {V_ROLES160,     4,  1,   2, 2, 5, 4, false, true},
};
// the row of variant id v, nullptr for a number that is no variant
constexpr const TileVariantInfo* tile_variant(int v) {
  for (const TileVariantInfo& t : TILE_VARIANTS)
    if (t.id == v) return &t;
  return nullptr;
}
static_assert(tile_variant(V_DB)->bm() == GBM && tile_variant(V_DB)->bn() == GBN && tile_variant(V_DB)->threads() == GNT);

// What icap_gemm launches for one call (shared by the launcher and icap_gemm_kernel_name).
struct GemmPlan {
  bool skinny = false;
  bool g256 = false;     // the 256 x 256 8-phase kernel (gemm256.hip)
  int g8p = 0;           // the 256-row 8-phase kernel (gemm8p.hip): its tile width BN (128 / 256), 0 = not taken
  int nt = 1;            // skinny: 16-column slabs per block
  int sku = 3;           // skinny: k-steps in flight per wave
  int variant = V_DB;    // tile kernel (TileVariant)
  int splits = 1, nk_split = 0, tiles_n = 0;
  bool fused = false;    // split-K combined inside the launch (tickets), no reduce pass
  int actk = ACT_ANY;    // tile kernels: the epilogue's activation instantiation (ACT_OFF / ACT_ANY / a specialised one)
  unsigned grid_x = 1, grid_y = 1, block_x = 1;  // (the launch sites build the dim3)
  uint32_t thr = 0;
  float inv_keep = 1.f;
};

// A/B overrides of the planner's rules. The product library holds the defaults as constants and reads no environment
// variable; the diagnostic build (make stamps: -DICAP_STAMPS) reads each from the variable named beside it
// (tools/ab, tools/gemm_tiles_ab.py).
struct PlanDiag {
  // short-K variant for launches with dact / aux, with an activation only, with neither
  int var_heavy = V_S3, var_act = V_S3, var_light = V_S3;  // ICAP_VAR_HEAVY / ICAP_VAR_ACT / ICAP_VAR_LIGHT
  int fused_s = 0;      // ICAP_FUSED_S > 1: that split count for the in-launch split-K (at most 4)
  int fused_nst = 0;    // ICAP_FUSED_NST: 1 = the in-launch split's K ranges take the variant rule, 4 = the 4-stage ring
  int fused_mink = 24;  // ICAP_FUSED_MINK >= 2: fewest K stages for the in-launch split
  int kskew = 1;        // ICAP_KSKEW: the K-skew (0 = off)
  bool kout_fused = false;  // ICAP_KOUT_FUSED = 1: K-outer weight-gradient splits combine in the launch
  bool spec_act = true;     // ICAP_SPEC_ACT = 0: the runtime-dispatch epilogue on every 128-row tile
  int force_tile = -1;  // ICAP_FORCE_TILE = 0 / 4 / 5 / 12 / 13 / 16: that variant for unsplit bf16 row-major launches
  int w192r = 4;        // ICAP_W192R = 2: never the ring form of the 192 x 64 tiles
};
PlanDiag plan_diag();

// The argument checks of one product (no kernel choice); ICAP_ERR_ARG and the error text on invalid arguments.
int gemm_validate(const icap_gemm_args& p);
// The plan for one call on a device of `cus` compute units; ICAP_ERR_ARG (and the error text) on invalid arguments.
int gemm_plan(const icap_gemm_args& p, GemmPlan& pl, int cus, const PlanDiag& diag = PlanDiag());
// K-skew of a tile-kernel launch of plan pl (0 = K in its natural order)
int gemm_plan_skew(const icap_gemm_args& p, const GemmPlan& pl, const PlanDiag& diag = PlanDiag());
// name of the kernel instantiation pl launches (a thread-local buffer)
const char* gemm_plan_kernel_name(const icap_gemm_args& a, const GemmPlan& pl);
// ICAP_ERR_ARG for a launcher that does not instantiate (pl.variant, pl.actk); the error text names both
int gemm_no_instantiation(const GemmPlan& pl);

}  // namespace icap
