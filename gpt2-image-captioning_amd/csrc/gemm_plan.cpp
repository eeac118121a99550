// The GEMM launch planner: which kernel instantiation, grid and split-K one icap_gemm call takes. Host-only (no
// HIP header; the planner never dereferences an operand pointer). gemm_plan validates the arguments, then tries one
// rule per kernel family in a fixed order; a family either fills the plan or passes. Which epilogue kinds a kernel has
// is not written here: every family reads its variant's row of gemm_plan.h's table of forms.
#include "gemm_plan.h"

#include <cstdio>

namespace icap {

PlanDiag plan_diag() {
  PlanDiag d;
  d.var_heavy = diag_env("ICAP_VAR_HEAVY", d.var_heavy);
  d.var_act = diag_env("ICAP_VAR_ACT", d.var_act);
  d.var_light = diag_env("ICAP_VAR_LIGHT", d.var_light);
  d.fused_s = diag_env("ICAP_FUSED_S", d.fused_s);
  d.fused_nst = diag_env("ICAP_FUSED_NST", d.fused_nst);
  if (const int v = diag_env("ICAP_FUSED_MINK", 0); v >= 2) d.fused_mink = v;
  d.kskew = diag_env("ICAP_KSKEW", d.kskew);
  d.kout_fused = diag_env("ICAP_KOUT_FUSED", 0) == 1;
  d.spec_act = diag_env("ICAP_SPEC_ACT", 1) != 0;
  d.force_tile = diag_env("ICAP_FORCE_TILE", d.force_tile);
  d.w192r = diag_env("ICAP_W192R", d.w192r);
  return d;
}

static bool al16(const void* ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 15) == 0; }
static int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
static bool plain(const icap_gemm_args& p) { return p.act == ICAP_ACT_NONE && p.dact == ICAP_ACT_NONE; }

int gemm_validate(const icap_gemm_args& p) {
  ICAP_REQUIRE(p.M >= 0 && p.N >= 0 && p.K >= 0, "icap_gemm: negative size");
  ICAP_REQUIRE(p.path == 0 || p.path == 1 || (p.path >= 3 && p.path <= 12), "icap_gemm: path must be 0, 1 or 3 ... 12");
  ICAP_REQUIRE(p.A && p.B && p.C, "icap_gemm: null operand");
  ICAP_REQUIRE(p.in_dtype == ICAP_F32 || p.in_dtype == ICAP_BF16 || p.in_dtype == ICAP_FP8_MX,
               "icap_gemm: bad in_dtype");
  ICAP_REQUIRE(p.c_dtype == ICAP_F32 || p.c_dtype == ICAP_BF16, "icap_gemm: bad c_dtype");
  const bool mx = p.in_dtype == ICAP_FP8_MX;
  if (mx) {
    ICAP_REQUIRE(p.K % 128 == 0 && p.lda % 16 == 0 && p.ldb % 16 == 0,
                 "icap_gemm: FP8_MX needs K % 128 == 0 and lda, ldb multiples of 16");
    ICAP_REQUIRE(p.a_scale && p.b_scale && al16(p.a_scale) && al16(p.b_scale),
                 "icap_gemm: FP8_MX needs 16-byte aligned a_scale / b_scale");
    ICAP_REQUIRE(!p.trans_ab && !p.ln_gamma && p.path != 3, "icap_gemm: FP8_MX takes no trans_ab / ln / path 3");
    ICAP_REQUIRE((p.K / 32) * ((p.M + 63) / 64) * 64 < 0x7fffffffll && (p.K / 32) * ((p.N + 63) / 64) * 64 < 0x7fffffffll,
                 "icap_gemm: FP8_MX scale arrays must stay below 2 GiB");
  }
  const int epc = p.in_dtype == ICAP_BF16 ? 8 : mx ? 16 : 4;
  ICAP_REQUIRE(p.trans_ab || p.K % epc == 0, "icap_gemm: K must be a multiple of 8 (bf16) / 4 (f32)");
  ICAP_REQUIRE(p.lda % epc == 0 && p.ldb % epc == 0, "icap_gemm: lda/ldb must be multiples of 8 (bf16) / 4 (f32)");
  ICAP_REQUIRE((p.trans_ab || (p.lda >= p.K && p.ldb >= p.K)) && p.ldc >= p.N, "icap_gemm: leading dimension too small");
  ICAP_REQUIRE((reinterpret_cast<uintptr_t>(p.A) & 15) == 0 && (reinterpret_cast<uintptr_t>(p.B) & 15) == 0,
               "icap_gemm: A and B must be 16-byte aligned");
  const int es = p.in_dtype == ICAP_BF16 ? 2 : mx ? 1 : 4;
  ICAP_REQUIRE((int64_t)256 * p.lda * es < 0x7fffffffll && (int64_t)256 * p.ldb * es < 0x7fffffffll,
               "icap_gemm: a 256-row operand panel must stay below 2 GiB");
  ICAP_REQUIRE(p.beta == 0.f || p.c_dtype == ICAP_F32, "icap_gemm: beta != 0 requires f32 C");
  ICAP_REQUIRE(p.dact == ICAP_ACT_NONE || p.dact_src != nullptr, "icap_gemm: dact requires dact_src");
  ICAP_REQUIRE(p.act >= ICAP_ACT_NONE && p.act <= ICAP_ACT_GELU_ERF && p.dact >= ICAP_ACT_NONE &&
                   p.dact <= ICAP_ACT_GELU_ERF, "icap_gemm: unknown activation");
  ICAP_REQUIRE(p.drop_p >= 0.f && p.drop_p < 1.f, "icap_gemm: drop_p out of range");
  if (p.trans_ab) {
    ICAP_REQUIRE(p.in_dtype == ICAP_BF16, "icap_gemm: trans_ab needs bf16 inputs");
    ICAP_REQUIRE(p.lda >= p.M && p.ldb >= p.N, "icap_gemm: trans_ab needs lda >= M, ldb >= N");
    ICAP_REQUIRE(p.m_dev == nullptr, "icap_gemm: trans_ab does not take m_dev");
    ICAP_REQUIRE((int64_t)(p.K + 64) * p.lda * 2 < 0x7fffffffll && (int64_t)(p.K + 64) * p.ldb * 2 < 0x7fffffffll,
                 "icap_gemm: trans_ab operands must stay below 2 GiB");
  }
  ICAP_REQUIRE(cdiv(p.M, GBM) * cdiv(p.N, GBN) < (1ll << 26), "icap_gemm: too many tiles");
  ICAP_REQUIRE(p.split_k >= 0, "icap_gemm: split_k must be >= 0");
  const bool fuse_ln = p.ln_gamma != nullptr;
  ICAP_REQUIRE(!fuse_ln || (p.ln_beta && p.M <= 128 && p.split_k == 0 && !p.trans_ab && p.K <= 4096),
               "icap_gemm: ln_gamma needs ln_beta, M <= 128, K <= 4096, no split_k / trans_ab");
  if (p.ln_stats_out || p.ln_stats_in) {  // the tile kernels' LayerNorm statistics hand-off
    ICAP_REQUIRE(p.in_dtype == ICAP_BF16 && p.c_dtype == ICAP_BF16 && !p.trans_ab && !fuse_ln && p.path != 3 &&
                     !(p.ln_stats_out && p.ln_stats_in) && p.beta == 0.f,
                 "icap_gemm: ln_stats_out / ln_stats_in: bf16 A/B/C, no trans_ab / ln_gamma / path 3 / beta, not both");
    ICAP_REQUIRE(!p.ln_stats_out || (p.N % 32 == 0 && plain(p)), "icap_gemm: ln_stats_out needs N % 32 == 0 and no activation");
    ICAP_REQUIRE(!p.ln_stats_in || (p.ln_wsum && p.K % 128 == 0 && p.K <= 1280 && p.dact == ICAP_ACT_NONE &&
                                    al16(p.ln_stats_in) && (p.ln_mean_out == nullptr) == (p.ln_rstd_out == nullptr)),
                 "icap_gemm: ln_stats_in needs ln_wsum, K % 128 == 0, K <= 1280, 16-byte aligned statistics, no dact, "
                 "ln_mean_out with ln_rstd_out");
  }
  const bool fold_ln = p.ln_wsum != nullptr && !p.ln_stats_in;  // (the skinny decode form: stats from A fragments)
  ICAP_REQUIRE(!fold_ln || (!fuse_ln && p.M <= 128 && p.split_k == 0 && !p.trans_ab && !mx && p.K <= 4096),
               "icap_gemm: ln_wsum needs M <= 128, no ln_gamma / split_k / trans_ab / FP8_MX, K <= 4096");
  return ICAP_OK;
}

// What every family's rule reads: the (valid, non-empty) call, the device, and the sizes derived from them once.
struct PlanCtx {
  const icap_gemm_args& p;
  const PlanDiag& diag;
  const int64_t cus;
  const bool mx = p.in_dtype == ICAP_FP8_MX;
  const bool lnx = p.ln_stats_out || p.ln_stats_in;  // the tile kernels' LayerNorm statistics hand-off
  const int64_t tiles_m = cdiv(p.M, GBM), tiles_n = cdiv(p.N, GBN), tiles = tiles_m * tiles_n;  // 128 x 128 tiles
  const int64_t nk = cdiv(p.K, 128 / (p.in_dtype == ICAP_BF16 ? 2 : mx ? 1 : 4));                // K stages of 128 bytes
  // with a device row count the kernel choice follows the expected count (m_hint)
  const int64_t m_plan = (p.m_dev && p.m_hint > 0 && p.m_hint < p.M) ? p.m_hint : p.M;
  const int64_t tiles_plan = cdiv(m_plan, GBM) * tiles_n;
};
// a family's answer: PASS = not its launch (the plan is untouched), else the return code of gemm_plan
constexpr int PASS = -1;

// ---- the helpers the families share -------------------------------------------------------------------------------

// `want` K ranges over nk stages: at most one per stage, every split gets >= 1 stage
struct SplitRanges {
  int64_t splits, nk_split;
};
static SplitRanges split_ranges(int64_t nk, int64_t want) {
  if (nk == 0) return {1, 0};
  const int64_t s = want < 1 ? 1 : want > nk ? nk : want;
  const int64_t nk_split = cdiv(nk, s);
  return {cdiv(nk, nk_split), nk_split};
}
// the fp32 slabs of a split that combines in the reduce pass
static int require_split_workspace(const icap_gemm_args& p, int64_t splits) {
  ICAP_REQUIRE((p.N & 3) == 0, "icap_gemm: split-K requires N % 4 == 0");
  ICAP_REQUIRE(p.workspace && (reinterpret_cast<uintptr_t>(p.workspace) & 15) == 0 &&
                   p.workspace_bytes >= splits * p.M * p.N * (int64_t)sizeof(float),
               "icap_gemm: split-K workspace missing, misaligned or too small");
  return ICAP_OK;
}

// The epilogue kind (ACT_* | ACT_LNS / ACT_LNF) of the launch on a kernel of capabilities c (a row of gemm_plan.h's
// table of forms), -1 where it has no form. Every kind it returns exists (epi_kind_exists; plan_check.cpp checks).
static int epilogue_kind(const icap_gemm_args& p, const EpiCaps& c) {
  const bool wide_c = p.c_dtype != ICAP_BF16 && c.f32_c_plain;
  int a = plain(p) ? ACT_OFF : ACT_ANY;
  if (a == ACT_ANY && p.in_dtype == ICAP_BF16 && !p.trans_ab && !wide_c) {
    if (p.dact == ICAP_ACT_NONE && (c.fwd & A_(p.act))) a = ACT_FWD + p.act;
    else if (p.act == ICAP_ACT_NONE && (c.bwd & A_(p.dact))) a = ACT_BWD + p.dact;
  }
  if (!p.ln_stats_out && !p.ln_stats_in) return a;
  if (wide_c) return -1;
  if (p.ln_stats_out) return (c.ln_producer && a == ACT_OFF) ? ACT_LNS + a : -1;
  if (!c.ln_consumer) return -1;
  const bool fwd_form = a > ACT_FWD && a < ACT_BWD && (c.ln_fwd & A_(a - ACT_FWD));
  return (a == ACT_OFF || fwd_form || (a == ACT_ANY && c.ln_any)) ? ACT_LNF + a : -1;
}
// what the ring families (gemm8p, variants 22 ... 32) take: bf16 row-major operands, no ln_gamma / decode fold
static bool ring_operands(const icap_gemm_args& p) {
  return p.in_dtype == ICAP_BF16 && !p.trans_ab && !p.ln_gamma && !(p.ln_wsum && !p.ln_stats_in);
}

// One tile-kernel launch of `splits` K ranges on variant v: tiles of v's size; the ring kernels at one block per CU
// walk the tiles (x splits), the others get one block per tile and split.
static void fill_tile_plan(const PlanCtx& c, GemmPlan& pl, int v, SplitRanges r, bool fused, int actk, bool walk) {
  const TileVariantInfo& t = *tile_variant(v);
  const int64_t tiles_n = cdiv(c.p.N, t.bn()), blocks = cdiv(c.p.M, t.bm()) * tiles_n * r.splits;
  pl.variant = v;
  pl.splits = (int)r.splits;
  pl.nk_split = (int)r.nk_split;
  pl.fused = fused;
  pl.tiles_n = (int)tiles_n;
  pl.actk = actk;
  pl.block_x = t.threads();
  pl.grid_x = (unsigned)(walk && blocks > c.cus ? c.cus : blocks);
}

// ---- the families, in the order gemm_plan tries them ---------------------------------------------------------------

// Skinny-M GEMM (M <= 128: greedy-decode steps over the batch, CLIP projection, mapper input Linear).
static int plan_skinny(const PlanCtx& c, GemmPlan& pl) {
  const icap_gemm_args& p = c.p;
  const bool fuse_ln = p.ln_gamma != nullptr, fold_ln = p.ln_wsum != nullptr && !p.ln_stats_in;
  if (!(p.M <= 128 && p.split_k == 0 && (c.tiles <= 128 || fuse_ln || fold_ln) && !p.trans_ab && !c.mx && !c.lnx)) return PASS;
  pl.skinny = true;
  // the fewest 16-column slabs per block that keep the grid within one pass over the CUs (every CU streams one
  // block's A rows + W slab; a second block on a CU doubles its bytes), then enough k-steps in flight per wave
  // to cover K in one round trip where the fragment registers allow (SKU in {3, 4, 6}; 12 for one-slab blocks)
  const int64_t gy = (p.M + 31) / 32;
  pl.nt = 4;
  for (int nt = 1; nt <= 4; ++nt)
    if (cdiv(p.N, 16 * nt) * gy <= c.cus) { pl.nt = nt; break; }
  if (p.in_dtype == ICAP_BF16) {
    const int64_t need = cdiv(cdiv(p.K, 32), SK_WAVES);
    pl.sku = need <= 3 ? 3 : need <= 4 ? 4 : (need <= 6 || pl.nt > 1) ? 6 : 12;
  } else {
    pl.sku = 6;
  }
  pl.grid_x = (unsigned)cdiv(p.N, 16 * pl.nt), pl.grid_y = (unsigned)gy;
  pl.block_x = 64 * SK_WAVES;
  return ICAP_OK;
}

// The 256 x 256 8-phase kernel (gemm256.hip) for wide products whose 256-tiles fill the chip in few, full rounds. It
// runs one block per CU, so a tile's prologue (first DMA round trip) and epilogue do not overlap other tiles' MFMAs:
// it beats the 128-row tile kernels (2-3 blocks per CU) on long K (4096^3: 1.09-1.22 vs 0.95 PF) and on many full
// tile rounds (LM head 8320 x 50304 x 768: 758 vs 835 us), not on the train step's 2-round K = 768 products (8320 x
// 3072 x 768: 84 vs 80 us) (profiles/r02_gemm256_bench.txt). path 3 forces it where eligible.
static int plan_g256(const PlanCtx& c, GemmPlan& pl) {
  const icap_gemm_args& p = c.p;
  if (p.path == 1 || (p.path >= 4 && p.path <= 12)) return PASS;
  if (p.in_dtype != ICAP_BF16 || p.trans_ab || p.ln_gamma || p.beta != 0.f || p.m_dev || p.split_k > 1) return PASS;
  if (c.lnx || p.M < 256 || p.N < 256 || p.K < 64) return PASS;
  if (p.path != 3) {
    const int64_t tiles = cdiv(p.M, 256) * cdiv(p.N, 256);
    const int64_t rounds = cdiv(tiles, c.cus);
    const bool full = tiles * 10 >= rounds * c.cus * 7;  // rounds at least 70 % occupied
    if (!((p.K >= 2048 && tiles * 4 >= c.cus * 3 && full) || (rounds >= 4 && tiles * 10 >= rounds * c.cus * 8))) return PASS;
  }
  pl.g256 = true;
  return ICAP_OK;
}

// The 256-row 8-phase kernel (gemm8p.hip) where its tiles fill the chip in one round: bf16 row-major operands, one K
// range (no split), the epilogue forms it instantiates (none / gelu_new fwd or bwd / any, the LayerNorm producer
// without an activation, the consumer without one or with gelu_new), for either C dtype. path 4 / 5 force its 128- /
// 256-column tiles where eligible.
static int plan_g8p(const PlanCtx& c, GemmPlan& pl) {
  const icap_gemm_args& p = c.p;
  if (!ring_operands(p) || p.split_k > 1) return PASS;
  if (p.M < 256 || p.K < 64 || p.path == 1 || p.path == 3 || p.path >= 6) return PASS;  // (6 ... 12: other forced forms)
  if (p.M * p.lda >= (1ll << 30) || p.N * p.ldb >= (1ll << 30)) return PASS;  // 32-bit DMA byte offsets per tile
  const int actk = epilogue_kind(p, G8P_EPI);
  if (actk < 0) return PASS;
  int bn = p.path == 4 ? 128 : p.path == 5 ? 256 : 0;
  if (bn == 0) {
    // one round of 256 x 256 tiles at least 80 % full, K <= 1536: there it beat every 128-row form (CLIP-B/32's
    // 6400 x 2304 x 768 QKV: 30.6 vs 38.6 us; x 1536: 47.6 vs 68.5); 256 x 128 tiles and other shapes did not
    // (the 3584-row products: within 3 %; N = 768: 30-60 % slower) — profiles/r05_g8p_ab.txt
    const int64_t t256 = cdiv(c.m_plan, 256) * cdiv(p.N, 256);
    // and (round 6) many rounds of them: the compact LM head, 1664 live rows x 50304 x 768 = 1379 tiles: 157 vs
    // 180 us on the 3-block 128 x 128 tiles (hipBLASLt 146; profiles/r06_lmhead_ab.txt)
    if (p.K <= 1536 && ((t256 * 10 >= c.cus * 8 && t256 <= c.cus) || t256 >= 4 * c.cus)) bn = 256;
  }
  if (bn == 0) return PASS;
  pl.g8p = bn;
  pl.actk = actk;
  return ICAP_OK;
}

// Variant 31 (round 6): the K-outer weight-gradient products on the split-role ring (4 MFMA + 4 LDS-DMA waves,
// 128 x 128 tiles, 4 stages, one block per CU), K split so tiles x splits fill about one round of CUs (a caller's
// split_k capped at 8; either lowered until every split has >= 4 stages), the splits combined by the slab + reduce
// pass. path 11 forces it for bf16 K-outer launches.
static int plan_roles_kout(const PlanCtx& c, GemmPlan& pl) {
  const icap_gemm_args& p = c.p;
  if (!(p.trans_ab && p.in_dtype == ICAP_BF16 && p.path == 11)) return PASS;
  ICAP_REQUIRE(p.K > 0, "icap_gemm: K must be positive");
  int64_t want = p.split_k >= 1 ? p.split_k : c.cus / c.tiles;
  if (want > 8) want = 8;
  while (want > 1 && c.nk / want < 4) --want;
  const SplitRanges r = split_ranges(c.nk, want);
  if (r.splits > 1)
    if (const int rc = require_split_workspace(p, r.splits); rc != ICAP_OK) return rc;
  fill_tile_plan(c, pl, V_ROLES_KOUT, r, false, plain(p) ? ACT_OFF : ACT_ANY, true);
  return ICAP_OK;
}

// The split of the 128-row tile kernels (the ring families below run unsplit, or on a caller's split_k, and read
// from it only whether the tile path would split).
struct TileSplit {
  int64_t splits = 1, nk_split = 0;
  bool fused = false;  // the splits combine inside the launch (tickets)
};
// enough tickets and partial-tile room for `want` splits to combine inside the launch
static bool fused_fits(const PlanCtx& c, int64_t want) {
  const int64_t pbytes = (int64_t)GBM * GBN * (int64_t)sizeof(float);
  // with a device row count the grid still covers every row tile of M, so tickets / partials for all of them
  return c.p.tickets && c.p.tickets_len >= 2 * c.tiles && c.p.workspace_bytes >= c.tiles * split_ranges(c.nk, want).splits * pbytes;
}
// Split-K over K stages for launches that cannot fill the chip (decode-time M = batch, small projections): fp32
// partial slabs in the caller's workspace + one deterministic reduce/epilogue pass — or, with tickets, the in-launch
// combine (long K over fewer tiles than CUs: the packed step's N = 768 products, the mapper's M = 3200 products and
// weight gradients): S = 2 * CUs / tiles rounded, 2..4, so the tile x split blocks fill the chip about twice, and no
// slab round trip or extra launch.
// The split count is a function of the shape (M, N, K, dtype, trans_ab; with a device row count, the caller's
// expected count m_hint) alone — never of the workspace size or of whether tickets are attached — so the partial
// sums are always added in the same order. Tickets only choose HOW the splits combine (inside the launch or in a
// reduce pass over slabs); both add the partials in split order starting from split 0 and apply the same epilogue
// formula, so the two mechanisms store bitwise-identical outputs (tests/test_fused_splitk_gpu.py). A NULL workspace
// turns the automatic split off (documented: include/icap.h); a given one too small for the shape's split is an error.
// Returns the wanted count; fusable = the long-K / few-tiles rule (the splits may combine inside the launch).
static int64_t wanted_splits(const PlanCtx& c, bool& fusable, bool& fused) {
  const icap_gemm_args& p = c.p;
  const int64_t nk = c.nk, tiles = c.tiles;
  fusable = fused = false;
  if (p.split_k > 1) return p.split_k;
  if (p.split_k == 1 || !p.workspace || (p.N & 3) != 0) return 1;
  // (not for the K-outer weight-gradient products: measured, their in-launch combine ran 6-7 µs slower than the
  // slab + reduce pass — 768x3072x3200 53 vs 47 µs, profiles/r03_gemm_detail_fused.txt — since the last arriver of
  // a 3-block-per-CU tile reads its partials one accumulator row at a time)
  if (!p.trans_ab && nk >= c.diag.fused_mink && c.tiles_plan < c.cus) {
    int64_t sf = (2 * c.cus + c.tiles_plan / 2) / c.tiles_plan;
    if (sf > 4) sf = 4;
    while (sf > 2 && nk / sf < 8) --sf;
    // A/B measurements only (ICAP_FUSED_S): the in-launch combine reads at most 3 other partials (4 splits)
    if (c.diag.fused_s > 1) sf = c.diag.fused_s < 4 ? c.diag.fused_s : 4;
    if (sf >= 2) {
      fusable = true;
      fused = fused_fits(c, sf);
      return sf;
    }
  }
  if (p.trans_ab && nk >= 16 && tiles < 320) {
    // K-outer weight gradients over the token rows (the mapper's 3200-row products): about 320 blocks, at most 6
    // splits — measured 31.8 / 23.3 / 35.4 / 35.8 us for 2304x768 / 768x768 / 3072x768 / 768x3072 over 3200 rows
    // against 33.9 / 24.7 / 40.3 / 40.2 with the 512-block rule below (profiles/r03_dw_bench.txt)
    int64_t s = cdiv(320, tiles);
    if (s > 6) s = 6;
    if (c.diag.kout_fused && s >= 2) {  // A/B only (ICAP_KOUT_FUSED=1): in-launch combine, at most 4 splits
      if (s > 4) s = 4;
      fused = fused_fits(c, s);
    }
    return s;
  }
  if (nk >= 2 && (tiles <= 64 || (tiles < 256 && nk >= 16))) {
    // the count depends on the shape alone — never on the workspace a caller passes — so a product computed on
    // another stream with its own scratch sums its K ranges in the same order and rounds identically (a
    // workspace too small for the shape's split is an error below, not a silent change of the summation order)
    int64_t s = cdiv(512, tiles);
    if (tiles > 64 && s > nk / 4) s = nk / 4;
    return s > 32 ? 32 : s;
  }
  return 1;
}
static int plan_tile_split(const PlanCtx& c, TileSplit& ts) {
  const icap_gemm_args& p = c.p;
  bool fusable;
  int64_t want = wanted_splits(c, fusable, ts.fused);
  // the LayerNorm statistics hand-off needs the full epilogue in the tile kernel: a split that could only combine
  // through the reduce pass is not taken (a rule of the call's arguments, so still one summation order per call)
  if (c.lnx && !fusable && p.split_k != 1) want = 1;
  const SplitRanges r = split_ranges(c.nk, want);
  ts.splits = r.splits, ts.nk_split = r.nk_split;
  if (ts.splits > 1 && !ts.fused)
    if (const int rc = require_split_workspace(p, ts.splits); rc != ICAP_OK) return rc;
  if (ts.fused)
    ICAP_REQUIRE((reinterpret_cast<uintptr_t>(p.workspace) & 15) == 0 && (reinterpret_cast<uintptr_t>(p.tickets) & 7) == 0,
                 "icap_gemm: split-K workspace / tickets misaligned");
  return ICAP_OK;
}

// The automatic choice of the split-role variants (0 = neither), one round of tiles at one block per CU (the kernel
// walks the tiles, but a second round pays a whole prologue / main loop / epilogue with nothing beside it). Measured
// against the automatic plan of round 5 (profiles/r06_roles_ab.txt, graph replay, packed rows): N <= 1024 on 96 x 128
// tiles — GPT-2 c_attn dX 3584 x 768 x 2304 30.5 -> 20.3 us, c_fc dX x 3072 33.9 -> 24.4, mlp c_proj fwd (+ LayerNorm
// statistics) 38.5 -> 28.1, attn c_proj 17.0 -> 14.4 / 12.4 -> 11.0, mapper 3200 x 768 x 3072 33.1 -> 25.3, CLIP fc2
// 6400 x 768 x 3072 (1.6 rounds, long K) 53.2 -> 48.2; CLIP's 6400 x 768 x 768 (1.6 rounds, short K) 20.4 -> 23.0: not
// taken. N > 1024 on 128 x 256 tiles where they fill one round: c_attn (LayerNorm consumer) 26.4 -> 24.5, mapper qkv
// 22.5 -> 19.9; the N = 3072 products (336 tiles: two rounds) 36.9 -> 45.1: not taken. Long K over fewer tiles
// (the LM-head dX, K = 50304 over 1792 rows) keeps the split-K kernels.
static int roles_pick(const PlanCtx& c) {
  const icap_gemm_args& p = c.p;
  const int64_t cus = c.cus, nk = c.nk;
  if (p.in_dtype != ICAP_BF16 || p.trans_ab || p.split_k > 1) return 0;
  if (p.N <= 1024) {
    const int64_t t = cdiv(c.m_plan, 96) * cdiv(p.N, 128);
    // more than one round of 96 x 128 tiles, one of 160 x 128 at least 80 % full: 160 x 128 (CLIP-B/32's 6400 x 768
    // out_proj / fc2 with the LayerNorm statistics: 240 tiles against 402, profiles/r06_roles160_ab.txt)
    const int64_t t160 = cdiv(c.m_plan, 160) * cdiv(p.N, 128);
    if (nk <= 96 && t > cus && t160 <= cus && t160 * 10 >= cus * 8) return V_ROLES160;
    if (nk > 96 || t * 5 < cus * 3) return 0;
    return (t <= cus || (nk >= 32 && 2 * t >= 3 * cus && t <= 2 * cus)) ? V_ROLES96 : 0;
  }
  // (one row tile — the greedy decode's LM head, 128 x 50304 — stays on the double-buffered tile loop below: 20.4
  // vs 21.9 us, profiles/r06_lmhead_dx_ab.txt)
  const int64_t t = cdiv(c.m_plan, 128) * cdiv(p.N, 256);
  return (c.m_plan > 128 && t <= cus && t * 5 >= cus * 3) ? V_ROLES : 0;
}
// Variants 26 / 27 / 28 / 32: the split-role ring (gemm_tile.h ROLES) on 128 x 256 / 96 x 128 / 192 x 256 / 160 x 128
// tiles, one K range per tile (path 8 / 9 / 10 / 12 force them where eligible; the automatic rule: roles_pick). 27 and
// 32 have no specialised activation and no LayerNorm consumer (their 96- / 160-row tiles do not pair two threads per
// row); 28 also has the relu forms.
static int plan_roles(const PlanCtx& c, GemmPlan& pl) {
  const icap_gemm_args& p = c.p;
  const int rv = p.path == 8 ? V_ROLES : p.path == 9 ? V_ROLES96 : p.path == 10 ? V_ROLES192 : p.path == 12 ? V_ROLES160
                 : p.path == 0 ? roles_pick(c) : 0;
  // a caller's split_k > 1 (the long-K LM head dX): K ranges over fp32 slabs + the reduce pass, as the tile path
  // (no LayerNorm hand-off: it needs the whole epilogue in the kernel)
  const bool rsplit = p.split_k > 1 && !c.lnx && rv != V_ROLES192;
  if (!rv || p.M < tile_variant(rv)->bm() || !(p.split_k <= 1 || rsplit) || !ring_operands(p)) return PASS;
  const int actk = epilogue_kind(p, tile_variant(rv)->epi);
  if (actk < 0) return PASS;
  if (rsplit) ICAP_REQUIRE(p.K > 0, "icap_gemm: K must be positive");
  const SplitRanges r = split_ranges(c.nk, rsplit ? p.split_k : 1);
  if (r.splits > 1)
    if (const int rc = require_split_workspace(p, r.splits); rc != ICAP_OK) return rc;
  fill_tile_plan(c, pl, rv, r, false, actk, true);  // the kernel walks the live tiles
  return ICAP_OK;
}

// Variant 22 (gemm_tile_r256.hip: 256 x 128 tiles, 8 waves, 3-stage ring, one block per CU), for an unsplit bf16
// row-major launch: path 6 forces it where eligible. The forms it instantiates: none, gelu_new fwd / bwd, quick_gelu
// fwd, any; the LayerNorm producer without an activation, the consumer without one or with gelu_new / quick_gelu.
static int plan_r256(const PlanCtx& c, const TileSplit& ts, GemmPlan& pl) {
  const icap_gemm_args& p = c.p;
  if (!(ts.splits == 1 && p.M >= 256 && p.path == 6 && ring_operands(p))) return PASS;
  const int actk = epilogue_kind(p, tile_variant(V_R256)->epi);
  if (actk < 0) return PASS;
  fill_tile_plan(c, pl, V_R256, split_ranges(c.nk, 1), false, actk, false);
  return ICAP_OK;
}

// Short-K launches (<= 16 stages) of fewer than 4 tiles of 128 x 128 per CU (the N = 768 products, the mapper's
// M = 3200 and CLIP's M = 6400 ones) run faster on 128 x 64 tiles: twice the blocks, so a CU holds more of them
// to hide each one's prologue / epilogue; longer K keeps 128 x 128 (profiles/r01_gemm_narrow.txt).
static bool narrow_tiles(const PlanCtx& c, const TileSplit& ts) {
  return c.p.in_dtype == ICAP_BF16 && c.p.M > 128 && !c.p.trans_ab && c.tiles < 1024 && c.nk <= 16 && ts.splits == 1;
}

// Variant 24: 192 x 64 tiles, unsplit (path 7 forces it where eligible): bf16 row-major operands, no LayerNorm fold /
// consumer; the statistics producer and activation-free launches get their own kinds, the rest the dispatching one.
// The automatic plan takes it for the products with N <= 1024 that run unsplit on 128 x 64 tiles (K <= 16 stages:
// 3584 / 3200 / 6400 x 768 x 768 — one round of 228 / 204 tiles instead of 1.3-2.6 rounds) or on 128 x 128 tiles
// filling one to two rounds (CLIP's 6400 x 768 x 3072), measured 0.7-1.6 and 5 us faster per launch
// (profiles/r05_w192_ab.txt); the long-K products that split K inside the launch stay there (33.9 vs 43.9 us on the
// mapper's 3200 x 768 x 3072). A LayerNorm statistics producer takes the kernel its plain product takes (equal C,
// tests/test_lnfold_gpu.py; 17.0 vs 17.1 us for GPT-2's attn c_proj)
static int plan_w192(const PlanCtx& c, const TileSplit& ts, GemmPlan& pl) {
  const icap_gemm_args& p = c.p;
  const int64_t cus = c.cus, t192 = cdiv(c.m_plan, 192) * cdiv(p.N, 64);
  bool w24 = p.path == 7;
  if (p.path == 0 && !p.ln_stats_in && p.N <= 1024 && p.in_dtype == ICAP_BF16 && !p.trans_ab && ts.splits == 1 && !ts.fused) {
    if (narrow_tiles(c, ts)) w24 = true;
    else if (ts.nk_split > 16 && !p.m_dev && c.tiles_plan >= cus && c.tiles_plan <= 2 * cus && t192 <= 2 * cus) w24 = true;
    // (Not for the launches that split K inside the launch: GPT-2's c_attn dX 3584 x 768 x 2304 runs 27.7-28.5 µs
    // unsplit on the 192 x 64 ring against 29.4-30.1 split in isolation, but the step with that rule measured 0.5 %
    // slower — 12833 / 12811 vs 12876 / 12895 images/s, profiles/r05_w192_ab.txt — so the split stays.)
  }
  if (!(w24 && p.M >= 192 && ring_operands(p))) return PASS;
  // K > 16 stages over one round of tiles: the 4-stage ring at one block per CU (ICAP_W192R = 2 in the
  // diagnostic build: never). Measured (profiles/r05_w192_ab.txt): GPT-2 c_attn dX 3584 x 768 x
  // 2304 28.1 µs on the ring, 33.0 double-buffered (29.4 with the automatic in-launch split-K); past one round
  // the double-buffered loop at 2 blocks per CU wins by far (CLIP fc2, 408 tiles: 48.2 vs 64.8 µs)
  const int v = c.nk > 16 && c.diag.w192r != 2 && t192 <= cus ? V_W192_RING : V_W192;
  const int actk = epilogue_kind(p, tile_variant(v)->epi);
  if (actk < 0) return PASS;
  fill_tile_plan(c, pl, v, split_ranges(c.nk, 1), false, actk, false);
  return ICAP_OK;
}

// Tile-kernel variant. Measured on MI355X (tools/gemm_bench.py, profiles/r01_gemm_variants.txt): short K (<= 16 stages) is
// bound by the per-block prologue/epilogue, which co-resident blocks hide -> single LDS buffer, 3-4 blocks/CU (4
// when the epilogue moves a second M x N tensor: dact_src read / aux store); long K favours the double-buffered
// main loop at 2 blocks/CU.
static int gemm_variant(const PlanCtx& c, int64_t nk_per_block) {
  if (nk_per_block > 16) return V_DB;
  const bool heavy = c.p.dact != ICAP_ACT_NONE || c.p.aux;
  // (A/B) ICAP_VAR_HEAVY / ICAP_VAR_ACT / ICAP_VAR_LIGHT: variant for short-K launches with dact / aux, with an
  // activation only, and with neither. Round 4: dact / aux launches at 3 blocks / CU too — the 4-block form (128
  // VGPRs) spills with those epilogues (profiles/r04_gemm_tiles_ab.txt: GPT-2 c_fc gelu + aux 42.2 vs 46.2 us,
  // mlp c_proj dgelu 43.4 vs 43.5)
  return heavy ? c.diag.var_heavy : !plain(c.p) ? c.diag.var_act : c.diag.var_light;
}
// the 128-row variant of a launch no ring family took
static int tile128_variant(const PlanCtx& c, const TileSplit& ts) {
  const icap_gemm_args& p = c.p;
  const bool bf16_rm = p.in_dtype == ICAP_BF16 && !p.trans_ab;
  int v = gemm_variant(c, ts.nk_split);
  // one row tile over many column tiles (the greedy decode's LM head, 128 x 50304 x 768): the double-buffered loop
  // (20.8 vs 22.8 µs, profiles/r05_lmhead_probe.txt)
  if (c.tiles_m == 1 && c.tiles_n > 256 && ts.splits == 1 && v == V_S3) v = V_DB;
  // in-launch split-K: the double-buffered main loop at 2 blocks per CU for every split's K range (measured on the
  // packed 3584 x 768 x 3072 / x 2304 products: 36.6 / 30.4 vs 40.1 / 32.4 µs with the single-stage form the
  // per-split K of 16 stages would pick; profiles/r03_fused_ab.txt); ICAP_FUSED_NST=1 restores the variant rule
  if (ts.fused && c.diag.fused_nst != 1) v = V_DB;
  // (A/B only) ICAP_FUSED_NST=4: the in-launch split-K on the 4-stage ring at one block per CU (three stages in
  // flight per CU instead of the double-buffered pair's two)
  if (ts.fused && c.diag.fused_nst == 4 && bf16_rm && !c.lnx) v = V_RING;
  // Long K over at most one 128 x 128 tile per CU and no split (no tickets given): the 4-stage ring at one block per
  // CU (the double-buffered loop at 2 blocks per CU only pays when a CU holds two tiles). Not for the LayerNorm
  // statistics hand-off (the ring has no such epilogue: GPT-2 large's 1280 x 1280 products at small batch).
  if (bf16_rm && ts.splits == 1 && ts.nk_split > 16 && c.tiles_plan <= c.cus && !c.lnx) v = V_RING;
  if (c.mx && v == V_S4) v = V_S3;  // MX at 4 blocks / CU (128 VGPRs) spills: 3 blocks / CU
  if (narrow_tiles(c, ts)) v = c.tiles_m * cdiv(p.N, 64) < 256 ? V_N12 : V_N13;
  if (p.trans_ab) v = ts.nk_split > 16 ? V_KOUT_DB : V_KOUT_S3;  // K-outer forms of variants 0 / 4
  // (diagnostic build) ICAP_FORCE_TILE = 0 / 4 / 5 / 12 / 13 / 16: that tile variant for unsplit bf16 row-major
  // launches. (Round 5 also tried 256 x 128 tiles of 8 waves on this template, double-buffered and single-buffered:
  // no faster on any of the step's shapes, profiles/r05_tile_graph_ab.txt; removed.)
  if (const int f = c.diag.force_tile; bf16_rm && ts.splits == 1 &&
      (f == V_DB || f == V_S3 || f == V_S4 || f == V_N12 || f == V_N13 || (f == V_RING && !c.lnx)))
    v = f;
  // the LayerNorm-folded quick_gelu consumer (CLIP c_fc) exists at 3 blocks / CU only (gemm_tile_ln.hip)
  if (c.lnx && v == V_DB && p.act == ICAP_ACT_QUICK_GELU) v = V_S3;
  return v;
}
// The epilogues of the 128-row tiles. The step's activated products get an epilogue compiled for their one activation
// (gemm_common.h ACT_FWD / ACT_BWD): GPT-2 c_fc gelu_new (+ aux) and its dgelu, CLIP c_fc quick_gelu, ViT / DINOv3
// c_fc erf gelu, the mapper's relu / drelu (128 x 64 tiles). Measured over the packed step (tools/ab/specact_ab.sh,
// profiles/r03_specact_ab.txt): 10.98 -> 10.61 ms; the mapper's 3200x3072x768 relu 36.4 -> 29.1 µs, CLIP's quick_gelu
// 68.6 -> 64.0, gelu + aux 64.5 -> 57.6 — the runtime dispatch over five activations (libm erff / tanhf / expf
// inlined per case) cost registers and scratch in the epilogue of every activated launch. The LayerNorm hand-off
// (gemm_tile_ln.hip): producers on 0 / 4 / 5 / 12 / 13; consumers there without an activation, with gelu_new on 0 / 4 /
// 5, quick_gelu on 4, and the dispatching form on 12 / 13.
static EpiCaps tile128_caps(int v, bool spec_act) {
  EpiCaps caps = tile_variant(v)->epi;
  if (!spec_act) caps.fwd = caps.bwd = 0;  // (diagnostic build) ICAP_SPEC_ACT = 0
  return caps;
}
// The 128-row tile kernels (variants 0 ... 16): every launch no other family took.
static int plan_tile128(const PlanCtx& c, const TileSplit& ts, GemmPlan& pl) {
  const bool in_kernel = ts.splits == 1 || ts.fused;  // (a reduce-pass split applies the epilogue in that pass)
  ICAP_REQUIRE(!c.lnx || in_kernel,
               "icap_gemm: ln_stats_* launches combine split-K inside the launch only (give the workspace tickets)");
  const int v = tile128_variant(c, ts);
  const int actk = in_kernel ? epilogue_kind(c.p, tile128_caps(v, c.diag.spec_act)) : ACT_OFF;
  ICAP_REQUIRE(actk >= 0, "icap_gemm: no LayerNorm-statistics form of the tile kernel this launch plans");
  fill_tile_plan(c, pl, v, {ts.splits, ts.nk_split}, ts.fused, actk, false);
  return ICAP_OK;
}

int gemm_plan(const icap_gemm_args& p, GemmPlan& pl, int cus, const PlanDiag& diag) {
  if (const int rc = gemm_validate(p); rc != ICAP_OK) return rc;
  pl.thr = p.drop_p > 0.f ? drop_threshold(p.drop_p) : 0u;
  pl.inv_keep = p.drop_p > 0.f ? 1.f / (1.f - p.drop_p) : 1.f;
  const PlanCtx c{p, diag, cus};
  if (p.M == 0 || p.N == 0) {  // nothing to launch (icap_gemm returns before planning): one K range, no rule runs
    pl.nk_split = (int)c.nk;
    return ICAP_OK;
  }
  int rc;
  if ((rc = plan_skinny(c, pl)) != PASS) return rc;
  if ((rc = plan_g256(c, pl)) != PASS) return rc;
  if ((rc = plan_g8p(c, pl)) != PASS) return rc;
  if ((rc = plan_roles_kout(c, pl)) != PASS) return rc;
  TileSplit ts;
  if ((rc = plan_tile_split(c, ts)) != ICAP_OK) return rc;
  if ((rc = plan_roles(c, pl)) != PASS) return rc;
  if ((rc = plan_r256(c, ts, pl)) != PASS) return rc;
  if ((rc = plan_w192(c, ts, pl)) != PASS) return rc;
  return plan_tile128(c, ts, pl);
}

// K-skew: tile (tm, tn) walks its K range starting at step ((7 tm + tn) * skew) mod nk and wraps, so the tiles of
// one XCD that share an A row panel (consecutive tn) or a B panel do not request the same lines in lockstep (a
// line they all miss on is fetched once and waited for by every one of them). Measured over the packed train step
// (eager per-shape table, profiles/r03_kskew_ab.txt): skew 1 took the N = 768 products 5-15 % shorter and the step
// 11.3 -> 10.9 ms; skew 2-4 less; launches over more than 64 k-steps per split (the LM-head dX, K = 50304) ran
// longer, so they keep the natural order. ICAP_KSKEW overrides the skew (0 = off; A/B only); path 1 (tile_only)
// keeps the natural order (the path-equality tests compare it bitwise with the 256 x 256 kernel).
int gemm_plan_skew(const icap_gemm_args& p, const GemmPlan& pl, const PlanDiag& diag) {
  const TileVariantInfo* t = tile_variant(pl.variant);
  if (t == nullptr || t->natural_k()) return 0;
  if (p.path == 1 || p.path >= 6 || p.in_dtype == ICAP_FP8_MX || pl.nk_split > 64) return 0;
  return diag.kskew > 0 && diag.kskew < 256 ? diag.kskew : 0;
}

const char* gemm_plan_kernel_name(const icap_gemm_args& a, const GemmPlan& pl) {
  static thread_local char buf[160];
  const char* ti = a.in_dtype == ICAP_BF16 ? "unsigned short" : a.in_dtype == ICAP_FP8_MX ? "icap::fp8_t" : "float";
  const char* tc = a.c_dtype == ICAP_BF16 ? "unsigned short" : "float";
  if (pl.g256) {
    snprintf(buf, sizeof buf, "icap::gemm256_kernel<%s>", tc);
  } else if (pl.g8p) {
    snprintf(buf, sizeof buf, "icap::gemm8p_kernel<%s, %d, %d>", tc, pl.g8p, pl.actk);
  } else if (pl.skinny) {
    snprintf(buf, sizeof buf, "icap::gemm_skinny_kernel<%s, %s, %d, 2, %d>", ti, tc, pl.nt, pl.sku);
  } else if (const TileVariantInfo* t = tile_variant(pl.variant)) {
    snprintf(buf, sizeof buf, "icap::gemm_kernel<%s, %s, %d, %d, %d, %d, %d, %d, %s, %d%s>", ti, tc, t->nst, t->minb, t->wm,
             t->wn, t->tm, t->tn, t->kout ? "true" : "false", pl.actk, t->roles ? ", true" : "");
  } else {
    return nullptr;
  }
  return buf;
}

int gemm_no_instantiation(const GemmPlan& pl) {
  set_error("icap_gemm: no instantiation of " + (pl.g8p ? "the 8-phase kernel of width " + std::to_string(pl.g8p)
                                                         : "tile variant " + std::to_string(pl.variant)) +
            " with epilogue kind " + std::to_string(pl.actk) + " for these dtypes");
  return ICAP_ERR_ARG;
}

GroupPlan gemm_group_plan(const int64_t* M, const int64_t* N, int n, int cus, bool force128) {
  GroupPlan big, small;
  big.big = true;
  for (int i = 0; i < n && i < GROUP_MAX; ++i) {
    const bool sw = N[i] <= GROUP_SWAP_N;
    const int64_t rows = sw ? N[i] : M[i], cols = sw ? M[i] : N[i];
    const int64_t bm = cdiv(rows, GROUP_BM), bn = cdiv(cols, GROUP_BN_BIG);
    const int64_t sm = cdiv(M[i], GBM), sn = cdiv(N[i], GBN);
    // (a product of more tiles than any one round holds only has to keep the sums and the casts in range)
    const int64_t cap = 1ll << 30;
    big.tiles_m[i] = (int)(bm < cap ? bm : cap), big.tiles_n[i] = (int)(bn < cap ? bn : cap);
    small.tiles_m[i] = (int)(sm < cap ? sm : cap), small.tiles_n[i] = (int)(sn < cap ? sn : cap);
    if (sw) big.swap |= 1u << i;
    big.total += (bm < cap && bn < cap && bm * bn < cap) ? bm * bn : cap;
    small.total += (sm < cap && sn < cap && sm * sn < cap) ? sm * sn : cap;
  }
  return (!force128 && big.total <= cus) ? big : small;
}

}  // namespace icap
