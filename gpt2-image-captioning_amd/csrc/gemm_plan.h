// The launch plan icap_gemm makes for one call, and the host-only planner that makes it (gemm_plan.cpp). No HIP
// dependency: the planner never dereferences an operand pointer, so a host compiler can exercise it without a GPU
// (plan_check.cpp).
#pragma once
#include "gemm_consts.h"
#include "host_common.h"

namespace icap {

// ---- the table of forms ----------------------------------------------------------------------------------------------
// Every instantiation of the tile kernel (gemm_tile.h gemm_kernel<TI, TC, NST, MINB, WM, WN, TM, TN, KOUT, ACT, ROLES>)
// and of the 256-row 8-phase kernel (gemm8p.hip gemm8p_kernel<TC, BN, ACT>) follows from TILE_VARIANTS / G8P_EPI below:
// the launchers instantiate exactly the forms tile_form_exists / g8p_form_exists name (gemm_launch.h, gemm8p.hip), the
// planner plans epilogue kinds from the same rows (gemm_plan.cpp epilogue_kind), and plan_check.cpp checks every plan
// against them. A new variant, input type or epilogue form is one edit of one row.

// Which epilogue instantiations a kernel has beside ACT_OFF and the runtime dispatch ACT_ANY. The specialised kinds and
// the LayerNorm hand-off exist for bf16 row-major operands only.
struct EpiCaps {
  unsigned fwd = 0, bwd = 0;  // bit a: ACT_FWD + a / ACT_BWD + a
  bool ln_producer = false;   // ACT_LNS (activation-free)
  bool ln_consumer = false;   // ACT_LNF, activation-free or with ...
  unsigned ln_fwd = 0;        // ... bit a: ACT_FWD + a
  bool ln_any = false;        // ... the runtime dispatch
  bool f32_c_plain = true;    // an fp32 C has ACT_OFF / ACT_ANY only
};
constexpr unsigned A_(int act) { return 1u << act; }
constexpr unsigned A_GN = A_(ICAP_ACT_GELU_NEW), A_QG = A_(ICAP_ACT_QUICK_GELU), A_RELU = A_(ICAP_ACT_RELU),
                   A_ERF = A_(ICAP_ACT_GELU_ERF);
constexpr unsigned IN_F32 = 1u << ICAP_F32, IN_BF16 = 1u << ICAP_BF16, IN_MX = 1u << ICAP_FP8_MX;  // input dtype sets

// The variants of the tile kernel, one row each. The ids are the numbers DESIGN.md, profiles/ and the tests use.
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
  unsigned in;   // the input dtypes it is instantiated for (IN_*)
  EpiCaps epi;   // its epilogue kinds
  constexpr int bm() const { return wm * tm * 16; }                          // tile rows
  constexpr int bn() const { return wn * tn * 16; }                          // tile columns
  constexpr int threads() const { return (wm * wn + (roles ? 4 : 0)) * 64; }  // (+ the 4 LDS-DMA waves)
  // the split-role variants walk K in its natural order (one round of tiles, no lockstep panel misses to stagger,
  // and automatic launches then equal forced ones and the tile path bitwise); the others take the K-skew
  constexpr bool natural_k() const { return roles; }
};
// Why a row has the kinds it has (measurements: gemm_plan.cpp tile128_caps, plan_roles, plan_r256, plan_w192): the
// 128 x 128 forms carry the step's activations (gelu_new everywhere, quick_gelu / erf gelu at 3 blocks / CU), the
// 128 x 64 forms the mapper's relu and the dispatching LayerNorm consumer; MX at 4 blocks / CU (128 VGPRs) spills, so
// V_S4 has none; the 96- / 160- / 192 x 64-row tiles do not pair two threads per row, so no LayerNorm consumer there.
constexpr unsigned IN_ALL = IN_BF16 | IN_F32 | IN_MX;
constexpr EpiCaps EPI_PLAIN = {}, EPI_LNS = {0, 0, true}, EPI_GELUS = {A_GN | A_QG, A_GN, true, true, A_GN | A_QG};
constexpr TileVariantInfo TILE_VARIANTS[] = {
    // id            NST MINB WM WN TM TN KOUT   ROLES  inputs            {fwd, bwd, LNS, LNF, LNF + fwd, LNF + any}
    {V_DB,           2,  2,   2, 2, 4, 4, false, false, IN_ALL,           {A_GN, A_GN, true, true, A_GN}},
    {V_S3,           1,  3,   2, 2, 4, 4, false, false, IN_ALL,           {A_GN | A_QG | A_ERF, A_GN, true, true, A_GN | A_QG}},
    {V_S4,           1,  4,   2, 2, 4, 4, false, false, IN_BF16 | IN_F32, {A_GN, A_GN, true, true, A_GN}},
    {V_N12,          2,  3,   2, 2, 4, 2, false, false, IN_BF16,          {0, 0, true, true, 0, true}},
    {V_N13,          1,  4,   2, 2, 4, 2, false, false, IN_BF16,          {A_RELU, A_RELU, true, true, 0, true}},
    {V_KOUT_DB,      2,  2,   2, 2, 4, 4, true,  false, IN_BF16,          EPI_PLAIN},
    {V_KOUT_S3,      1,  3,   2, 2, 4, 4, true,  false, IN_BF16,          EPI_PLAIN},
    {V_RING,         4,  1,   2, 2, 4, 4, false, false, IN_BF16,          EPI_PLAIN},
    {V_R256,         3,  1,   4, 2, 4, 4, false, false, IN_BF16,          EPI_GELUS},
    {V_W192,         2,  2,   4, 1, 3, 4, false, false, IN_BF16,          EPI_LNS},
    {V_W192_RING,    4,  1,   4, 1, 3, 4, false, false, IN_BF16,          EPI_LNS},
    {V_ROLES,        3,  1,   2, 2, 4, 8, false, true,  IN_BF16,          EPI_GELUS},
    {V_ROLES96,      5,  1,   2, 2, 3, 4, false, true,  IN_BF16,          EPI_LNS},
    {V_ROLES192,     2,  1,   2, 4, 6, 4, false, true,  IN_BF16,          {A_GN | A_QG | A_RELU, A_GN | A_RELU, true, true, A_GN | A_QG}},
    {V_ROLES_KOUT,   4,  1,   2, 2, 4, 4, true,  true,  IN_BF16,          EPI_PLAIN},
    {V_ROLES160,     4,  1,   2, 2, 5, 4, false, true,  IN_BF16,          EPI_LNS},
};
// the row of variant id v, nullptr for a number that is no variant
constexpr const TileVariantInfo* tile_variant(int v) {
  for (const TileVariantInfo& t : TILE_VARIANTS)
    if (t.id == v) return &t;
  return nullptr;
}
static_assert(tile_variant(V_DB)->bm() == GBM && tile_variant(V_DB)->bn() == GBN && tile_variant(V_DB)->threads() == GNT);
// The 8-phase kernel: bf16 row-major operands, tiles of 128 or 256 columns, these kinds for either C dtype.
constexpr EpiCaps G8P_EPI = {A_GN, A_GN, true, true, A_GN, false, false};
constexpr int G8P_WIDTHS[] = {128, 256};

// The finite list of epilogue kinds: {none, ACT_LNS, ACT_LNF} x {ACT_OFF, ACT_ANY, ACT_FWD + a, ACT_BWD + a}.
constexpr int N_ACTS = ICAP_ACT_GELU_ERF, N_EPI_KINDS = 3 * (2 + 2 * N_ACTS);
constexpr int epi_kind_at(int i) {
  const int ln = i / (2 + 2 * N_ACTS), j = i % (2 + 2 * N_ACTS);
  return (ln == 0 ? 0 : ln == 1 ? ACT_LNS : ACT_LNF) + (j < 2 ? j : j < 2 + N_ACTS ? ACT_FWD + j - 1 : ACT_BWD + j - 1 - N_ACTS);
}
static_assert(epi_kind_at(0) == ACT_OFF && epi_kind_at(1) == ACT_ANY && epi_kind_at(2) == ACT_FWD + ICAP_ACT_GELU_NEW &&
              epi_kind_at(N_EPI_KINDS - 1) == ACT_LNF + ACT_BWD + ICAP_ACT_GELU_ERF);
// whether a kernel of capabilities c has epilogue kind actk, for bf16 row-major operands or others, a bf16 or fp32 C
constexpr bool epi_kind_exists(const EpiCaps& c, bool bf16_rm, bool c_bf16, int actk) {
  const int ln = actk & ~0xFF, a = actk & 0xFF;
  const bool fwd = a > ACT_FWD && a <= ACT_FWD + N_ACTS, bwd = a > ACT_BWD && a <= ACT_BWD + N_ACTS;
  const bool special = bf16_rm && (c_bf16 || !c.f32_c_plain);  // more than ACT_OFF / ACT_ANY
  if (ln == 0) return a == ACT_OFF || a == ACT_ANY || (special && ((fwd && (c.fwd & A_(a - ACT_FWD))) || (bwd && (c.bwd & A_(a - ACT_BWD)))));
  if (!special) return false;
  if (ln == ACT_LNS) return c.ln_producer && a == ACT_OFF;
  if (ln == ACT_LNF) return c.ln_consumer && (a == ACT_OFF || (a == ACT_ANY && c.ln_any) || (fwd && (c.ln_fwd & A_(a - ACT_FWD))));
  return false;
}
// whether gemm_kernel is instantiated for variant v, these dtypes and epilogue kind actk
constexpr bool tile_form_exists(int v, int in_dtype, int c_dtype, int actk) {
  const TileVariantInfo* t = tile_variant(v);
  if (t == nullptr || in_dtype < ICAP_F32 || in_dtype > ICAP_FP8_MX || !(t->in >> in_dtype & 1)) return false;
  if (c_dtype != ICAP_F32 && c_dtype != ICAP_BF16) return false;
  return epi_kind_exists(t->epi, in_dtype == ICAP_BF16 && !t->kout, c_dtype == ICAP_BF16, actk);
}
// whether gemm8p_kernel is instantiated for tiles of bn columns, this C dtype and epilogue kind actk
constexpr bool g8p_form_exists(int bn, int c_dtype, int actk) {
  return (bn == G8P_WIDTHS[0] || bn == G8P_WIDTHS[1]) && (c_dtype == ICAP_F32 || c_dtype == ICAP_BF16) &&
         epi_kind_exists(G8P_EPI, true, c_dtype == ICAP_BF16, actk);
}

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
// ICAP_ERR_ARG for a launch whose form does not exist (tile_form_exists / g8p_form_exists); the error text names it
int gemm_no_instantiation(const GemmPlan& pl);

// The tile choice of one grouped launch (icap_gemm_group, round 10). A group takes the split-role K-outer body on
// 128 x 256 tiles (big) when its tiles then fit ONE round of one block per compute unit, total <= cus; otherwise, or
// with force128 (the ICAP_GROUP128 override), it keeps the 128 x 128 body and walks total tiles on min(total, cus)
// blocks. On the big tiles a product with at most GROUP_SWAP_N output columns (a bias gradient dY^T . ones) runs with
// its operands exchanged (swap bit i): the narrow operand on the tile's 128 rows, the wide one on its 256 columns, the
// tile stored transposed — ceil(M / 256) tiles instead of ceil(M / 128). Every K-outer shape gemm_validate accepts
// fits either tile (columns past M / N are read and never stored), so the round count is the only condition.
constexpr int GROUP_MAX = 8, GROUP_BM = 128, GROUP_BN_BIG = 256, GROUP_SWAP_N = 4;
struct GroupPlan {
  bool big = false;            // 128 x 256 tiles (gemm_group256_kernel); else 128 x 128 (gemm_group_kernel)
  unsigned swap = 0;           // bit i: product i runs with A and B exchanged (big only)
  int tiles_m[GROUP_MAX] = {}, tiles_n[GROUP_MAX] = {};  // per product, of the orientation it runs in
  int64_t total = 0;           // tiles of the whole group
};
// n <= GROUP_MAX products of M[i] x N[i] outputs (all positive)
GroupPlan gemm_group_plan(const int64_t* M, const int64_t* N, int n, int cus, bool force128);

}  // namespace icap
