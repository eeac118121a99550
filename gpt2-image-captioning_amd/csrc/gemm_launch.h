// The launchers of the tile kernel (gemm_tile_*.hip: one translation unit per group of forms, so their instantiations
// compile in parallel) and the one generic launcher they are written with: it instantiates what gemm_plan.h's table
// of forms names, nothing else.
#pragma once
#include <utility>

#include "gemm_plan.h"
#include "gemm_tile.h"

namespace icap {
// Launch the tile-kernel instantiation pl selects (grid pl.grid_x, block pl.block_x); nks = nk_split | skew / diag
// bits. ICAP_ERR_ARG (gemm_no_instantiation) for a form that does not exist or is not the unit's.
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
  unsigned swap;  // (128 x 256 tiles) bit i: a[i] holds the product with A and B exchanged, its tiles store C^T
};
// big: the 128 x 256 tiles of gemm_group256_kernel (the host's gemm_group_plan: the group then fits one round)
void launch_group_kout(const GemmGroup& g, int cus, bool big, hipStream_t s);

// The epilogue kinds a unit holds: the 128-row variants spread theirs over three units (gemm.hip tile_launcher).
enum KindSet : int { KINDS_PLAIN = 1, KINDS_ACT = 2, KINDS_LN = 4, KINDS_ALL = 7 };
constexpr int kind_set(int actk) { return actk >= ACT_LNS ? KINDS_LN : actk >= ACT_FWD ? KINDS_ACT : KINDS_PLAIN; }

// Variant V with epilogue kind KIND, if that form exists (tile_form_exists), is one of the unit's KINDS and pl asks for
// it; the template numbers are V's row of TILE_VARIANTS.
template <typename TI, typename TC, int V, int KINDS, int KIND>
bool launch_tile_form(const GemmPlan& pl, const icap_gemm_args& p, int nks, hipStream_t s) {
  if constexpr ((kind_set(KIND) & KINDS) != 0 && tile_form_exists(V, dtype_of<TI>, dtype_of<TC>, KIND)) {
    if (pl.actk != KIND) return false;
    constexpr TileVariantInfo t = *tile_variant(V);
    hipLaunchKernelGGL((gemm_kernel<TI, TC, t.nst, t.minb, t.wm, t.wn, t.tm, t.tn, t.kout, KIND, t.roles>),
                       dim3(pl.grid_x, pl.grid_y), dim3(pl.block_x), 0, s, p, pl.tiles_n, pl.splits, nks, pl.thr, pl.inv_keep);
    return true;
  }
  return false;
}
template <typename TI, typename TC, int V, int KINDS, int... I>
bool launch_tile_kinds(const GemmPlan& pl, const icap_gemm_args& p, int nks, hipStream_t s, std::integer_sequence<int, I...>) {
  return (launch_tile_form<TI, TC, V, KINDS, epi_kind_at(I)>(pl, p, nks, s) || ...);
}
// The generic launcher: the forms of variants V... with input type TI, either C dtype, and the kinds of set KINDS.
template <typename TI, int KINDS, int... V>
int launch_tile_forms(const GemmPlan& pl, const icap_gemm_args& p, int nks, hipStream_t s) {
  constexpr auto kinds = std::make_integer_sequence<int, N_EPI_KINDS>();
  const bool c16 = p.c_dtype == ICAP_BF16;
  const bool done = ((pl.variant == V && (c16 ? launch_tile_kinds<TI, bf16_t, V, KINDS>(pl, p, nks, s, kinds)
                                              : launch_tile_kinds<TI, float, V, KINDS>(pl, p, nks, s, kinds))) || ...);
  return done ? ICAP_OK : gemm_no_instantiation(pl);
}

}  // namespace icap

