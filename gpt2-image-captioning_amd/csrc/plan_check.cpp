// Stand-alone host check of the GEMM launch planner (gemm_plan.cpp): sweeps shapes and arguments at 256 compute units
// with fake aligned pointers (the planner never dereferences one), asserts each plan's invariants and prints one
// FNV-1a hash over (return code, error text or every GemmPlan field, K-skew, kernel name) of all cases. Built by
// `make plan_check` with the host compiler under ASan + UBSan; tests/test_gemm_plan_cpu.py pins the hashes.
//
// It also asserts that every tile or 8-phase plan names a form gemm_plan.h's table of forms has (tile_form_exists /
// g8p_form_exists: what the launchers instantiate), so a planner / launcher mismatch stops here and not at a GPU launch.
//
// Three hashes: "pinned" leaves out the inputs on which the rules before the planner was restructured divided by zero
// (nothing to launch: M or N = 0; K = 0 on path 11, or on paths 8 / 9 / 12 with split_k > 1), so it is comparable
// across that restructuring; "all" includes them; "diag" is the third sweep's, under the PlanDiag overrides. Then the
// coverage: how many of the table's forms some case planned (exit code 1 if one that can be planned never was) and,
// line by line, the forms planned only under a non-default PlanDiag.
#include "gemm_plan.h"

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

static thread_local std::string g_err;
namespace icap {
void set_error(const std::string& msg) { g_err = msg; }
}  // namespace icap
using namespace icap;

// whether this build plans the inputs on which the unrestructured rules divided by zero (-DPLAN_CHECK_ALL_INPUTS=0:
// leave them out, to run the check on those rules)
#ifndef PLAN_CHECK_ALL_INPUTS
#define PLAN_CHECK_ALL_INPUTS 1
#endif
static constexpr int CUS = 256;

struct Fnv {
  uint64_t h = 1469598103934665603ull;
  void bytes(const void* p, size_t n) {
    const unsigned char* c = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ c[i]) * 1099511628211ull;
  }
  void i64(int64_t v) { bytes(&v, sizeof v); }
  void str(const char* s) { bytes(s, std::strlen(s) + 1); }
};

// The forms of gemm_plan.h's table, numbered: tile (row of TILE_VARIANTS, in_dtype, c_dtype, kind), then 8-phase (width,
// c_dtype, kind). Most slots hold no form (tile_form_exists / g8p_form_exists).
static constexpr int N_VAR = sizeof TILE_VARIANTS / sizeof *TILE_VARIANTS;
static constexpr int N_TILE_SLOTS = N_VAR * 3 * 2 * N_EPI_KINDS, N_SLOTS = N_TILE_SLOTS + 2 * 2 * N_EPI_KINDS;
enum : unsigned char { PLANNED = 1, PLANNED_DEFAULT = 2 };
struct Form {
  bool g8p;
  int variant_or_bn, in_dtype, c_dtype, actk;
  bool exists() const {
    return g8p ? g8p_form_exists(variant_or_bn, c_dtype, actk) : tile_form_exists(variant_or_bn, in_dtype, c_dtype, actk);
  }
};
static Form form_of_slot(int slot) {
  const bool g8p = slot >= N_TILE_SLOTS;
  if (g8p) slot -= N_TILE_SLOTS;
  const int actk = epi_kind_at(slot % N_EPI_KINDS), c_dtype = slot / N_EPI_KINDS % 2, hi = slot / N_EPI_KINDS / 2;
  if (g8p) return {true, G8P_WIDTHS[hi], ICAP_BF16, c_dtype, actk};
  return {false, TILE_VARIANTS[hi / 3].id, hi % 3, c_dtype, actk};
}
// the slot of a form that exists, -1 for one that does not
static int slot_of_form(const Form& f) {
  if (!f.exists()) return -1;
  int k = 0;
  while (epi_kind_at(k) != f.actk) ++k;
  if (f.g8p) return N_TILE_SLOTS + ((f.variant_or_bn == G8P_WIDTHS[1]) * 2 + f.c_dtype) * N_EPI_KINDS + k;
  return (((int)(tile_variant(f.variant_or_bn) - TILE_VARIANTS) * 3 + f.in_dtype) * 2 + f.c_dtype) * N_EPI_KINDS + k;
}
static_assert(ICAP_F32 == 0 && ICAP_BF16 == 1 && ICAP_FP8_MX == 2);
// The 8-phase kernel is instantiated with the LayerNorm hand-off for either C dtype, and gemm_validate takes the
// hand-off with a bf16 C only: no call can plan these six forms.
static bool unplannable(const Form& f) { return f.g8p && f.c_dtype == ICAP_F32 && f.actk >= ACT_LNS; }
static std::string form_name(const Form& f) {
  icap_gemm_args a;
  std::memset(&a, 0, sizeof a);
  a.in_dtype = f.in_dtype, a.c_dtype = f.c_dtype;
  GemmPlan pl;
  pl.actk = f.actk;
  if (f.g8p) pl.g8p = f.variant_or_bn;
  else pl.variant = f.variant_or_bn;
  return gemm_plan_kernel_name(a, pl);
}

struct Job {
  Fnv pinned, all, diag;
  int64_t n_pinned = 0, n_all = 0, n_skipped = 0, n_diag = 0;
  bool default_diag = true;               // its cases run under the default PlanDiag
  unsigned char planned[N_SLOTS] = {};    // per form: PLANNED, PLANNED_DEFAULT
};

template <typename T>
static T* fake(uintptr_t v) { return reinterpret_cast<T*>(v); }

static icap_gemm_args base_args(int64_t M, int64_t N, int64_t K, int trans, int in_dtype, int c_dtype) {
  icap_gemm_args a;
  std::memset(&a, 0, sizeof a);
  a.M = M, a.N = N, a.K = K;
  a.in_dtype = in_dtype, a.c_dtype = c_dtype;
  a.A = a.B = fake<void>(1u << 20);
  a.C = fake<void>(1u << 20);
  a.lda = trans ? (M + 7) / 8 * 8 : K;
  a.ldb = trans ? (N + 7) / 8 * 8 : K;
  a.ldc = N;
  a.alpha = 1.f;
  a.trans_ab = trans;
  a.ln_eps = 1e-5f;
  if (in_dtype == ICAP_FP8_MX) a.a_scale = a.b_scale = fake<const uint8_t>(1u << 23);
  return a;
}
static void give_scratch(icap_gemm_args& a, bool ws, bool tickets) {
  if (ws) a.workspace = fake<void>(1u << 21), a.workspace_bytes = 1ll << 40;
  if (tickets) a.tickets = fake<int32_t>(1u << 22), a.tickets_len = 1ll << 30;
}

static bool crash_input(const icap_gemm_args& a) {
  if (a.M == 0 || a.N == 0) return true;
  if (a.K != 0) return false;
  return a.path == 11 || ((a.path == 8 || a.path == 9 || a.path == 12) && a.split_k > 1);
}

[[noreturn]] static void fail(const icap_gemm_args& a, const GemmPlan& pl, const char* what) {
  std::fprintf(stderr,
               "plan_check: %s: M %lld N %lld K %lld in %d c %d trans %d path %d split_k %d ws %d tickets %d beta %g act %d "
               "dact %d aux %d lnso %d lnsi %d lng %d lnw %d m_dev %d m_hint %lld drop %g -> skinny %d g256 %d g8p %d variant %d "
               "splits %d nk_split %d grid %u %u block %u fused %d\n",
               what, (long long)a.M, (long long)a.N, (long long)a.K, a.in_dtype, a.c_dtype, a.trans_ab, a.path, a.split_k,
               a.workspace != nullptr, a.tickets != nullptr, a.beta, a.act, a.dact, a.aux != nullptr,
               a.ln_stats_out != nullptr, a.ln_stats_in != nullptr, a.ln_gamma != nullptr, a.ln_wsum != nullptr,
               a.m_dev != nullptr, (long long)a.m_hint, a.drop_p, pl.skinny, pl.g256, pl.g8p, pl.variant, pl.splits,
               pl.nk_split, pl.grid_x, pl.grid_y, pl.block_x, pl.fused);
  std::exit(1);
}

// One case: plan it, check the plan, hash it. With a PlanDiag (sweep 3) the case goes into the "diag" hash, else into
// "pinned" / "all".
static void run_case(const icap_gemm_args& a, Job& job, const PlanDiag* diag = nullptr) {
  const PlanDiag dflt;
  const PlanDiag& d = diag ? *diag : dflt;
  const bool crash = crash_input(a);
  if (crash && !PLAN_CHECK_ALL_INPUTS) {
    ++job.n_skipped;
    return;
  }
  g_err.clear();
  GemmPlan pl;
  const int rc = gemm_plan(a, pl, CUS, d);
  Fnv h;
  h.i64(rc);
  if (rc != ICAP_OK) {
    h.str(g_err.c_str());
  } else {
    const bool tile = !pl.skinny && !pl.g256 && !pl.g8p;
    const int64_t stage = a.in_dtype == ICAP_BF16 ? 64 : a.in_dtype == ICAP_FP8_MX ? 128 : 32;
    const int64_t nk = (a.K + stage - 1) / stage;
    if (pl.splits < 1) fail(a, pl, "splits < 1");
    if (tile && (int64_t)pl.splits * pl.nk_split < nk) fail(a, pl, "the splits do not cover the K stages");
    if (a.M > 0 && a.N > 0 && (pl.grid_x == 0 || pl.grid_y == 0 || pl.block_x == 0)) fail(a, pl, "empty grid or block");
    if (pl.fused && (a.tickets == nullptr || a.workspace == nullptr)) fail(a, pl, "fused without tickets");
    const int64_t f[] = {pl.skinny, pl.g256, pl.g8p, pl.nt, pl.sku, pl.variant, pl.splits, pl.nk_split, pl.tiles_n,
                         pl.fused, pl.actk, pl.grid_x, pl.grid_y, pl.block_x, pl.thr, gemm_plan_skew(a, pl, d)};
    h.bytes(f, sizeof f);
    h.bytes(&pl.inv_keep, sizeof pl.inv_keep);
    h.str(gemm_plan_kernel_name(a, pl));
    if (tile || pl.g8p) {  // the launcher instantiates what the planner planned
      const int slot = slot_of_form({pl.g8p != 0, pl.g8p ? pl.g8p : pl.variant, a.in_dtype, a.c_dtype, pl.actk});
      if (slot < 0) fail(a, pl, "the table of forms has no such instantiation");
      job.planned[slot] |= job.default_diag ? PLANNED | PLANNED_DEFAULT : PLANNED;
    }
  }
  if (diag) {
    job.diag.i64((int64_t)h.h);
    ++job.n_diag;
    return;
  }
  job.all.i64((int64_t)h.h);
  ++job.n_all;
  if (!crash) {
    job.pinned.i64((int64_t)h.h);
    ++job.n_pinned;
  }
}

// sweep 1: shapes x paths x layouts x split_k x dtypes x scratch x beta
static const int64_t M1[] = {0, 1, 95, 96, 97, 128, 129, 160, 192, 256, 257, 1664, 1792, 3200, 3584, 6400, 8320};
static const int64_t N1[] = {0, 4, 60, 64, 102, 256, 768, 1024, 1028, 1280, 2304, 3072, 50304};
static const int64_t K1[] = {0, 8, 64, 128, 768, 1024, 1032, 1536, 1544, 2048, 2304, 3072, 4096, 6144, 6208, 50304};
static const int SPLIT1[] = {0, 1, 2, 3, 9};

static void sweep1(int64_t M, Job& job) {
  for (int64_t N : N1)
    for (int64_t K : K1)
      for (int path = 0; path <= 13; ++path)
        for (int trans = 0; trans <= 1; ++trans)
          for (int split_k : SPLIT1)
            for (int in_dtype : {ICAP_F32, ICAP_BF16, ICAP_FP8_MX})
              for (int c_dtype : {ICAP_F32, ICAP_BF16})
                for (int scratch = 0; scratch < 4; ++scratch)
                  for (int beta = 0; beta <= 1; ++beta) {
                    icap_gemm_args a = base_args(M, N, K, trans, in_dtype, c_dtype);
                    a.path = path;
                    a.split_k = split_k;
                    a.beta = (float)beta;
                    give_scratch(a, scratch & 1, scratch & 2);
                    run_case(a, job);
                  }
}

// sweep 2: the epilogue axes on the train step's shapes (bf16 row-major operands)
static const int64_t M2[] = {128, 1664, 3200, 3584, 6400, 8320};
static const int64_t NK2[] = {768, 2304, 3072};
static const int PATH2[] = {0, 1, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12};
enum { LN_NONE, LN_STATS_OUT, LN_STATS_IN, LN_GAMMA, LN_WSUM, LN_MODES };

static void sweep2(int64_t M, Job& job) {
  for (int64_t N : NK2)
    for (int64_t K : NK2)
      for (int path : PATH2)
        for (int act = ICAP_ACT_NONE; act <= ICAP_ACT_GELU_ERF; ++act)
          for (int dact = ICAP_ACT_NONE; dact <= ICAP_ACT_GELU_ERF; ++dact)
            for (int aux = 0; aux <= 1; ++aux)
              for (int ln = 0; ln < LN_MODES; ++ln)
                for (int mdev = 0; mdev < 3; ++mdev)
                  for (int drop = 0; drop <= 1; ++drop)
                    for (int c_dtype : {ICAP_F32, ICAP_BF16})
                      for (int scratch = 0; scratch <= 1; ++scratch) {
                        icap_gemm_args a = base_args(M, N, K, 0, ICAP_BF16, c_dtype);
                        a.path = path;
                        a.act = act;
                        a.dact = dact;
                        if (dact != ICAP_ACT_NONE) a.dact_src = fake<void>(1u << 24), a.ld_dact = N;
                        if (aux) a.aux = fake<void>(1u << 25), a.ldaux = N;
                        if (ln == LN_STATS_OUT) a.ln_stats_out = fake<float>(1u << 26);
                        if (ln == LN_STATS_IN) a.ln_stats_in = fake<const float>(1u << 26);
                        if (ln == LN_STATS_IN || ln == LN_WSUM) a.ln_wsum = fake<const float>(1u << 27);
                        if (ln == LN_GAMMA) a.ln_gamma = a.ln_beta = fake<const float>(1u << 27);
                        if (mdev) a.m_dev = fake<const int32_t>(1u << 28), a.m_hint = mdev == 2 ? 3584 : 0;
                        a.drop_p = drop ? 0.1f : 0.f;
                        give_scratch(a, scratch, scratch);
                        run_case(a, job);
                      }
}

// sweep 3: what the first two leave out — fp32 / MX / K-outer operands with activations and the LayerNorm hand-off,
// each under the PlanDiag overrides of the diagnostic build (one job per override; diag3(0) is the default)
static PlanDiag diag3(int i) {
  PlanDiag d;
  if (i == 1) d.var_heavy = d.var_act = d.var_light = V_S4;
  if (i == 2) d.var_heavy = d.var_act = d.var_light = V_DB;
  constexpr int force[] = {V_DB, V_S3, V_S4, V_N12, V_N13, V_RING};
  if (i >= 3 && i < 9) d.force_tile = force[i - 3];
  if (i == 9) d.spec_act = false;
  if (i == 10) d.fused_nst = 1;
  if (i == 11) d.fused_nst = 4;
  return d;
}
static constexpr int N_DIAG3 = 12;
static const int64_t M3[] = {128, 3584, 8320};
static const int64_t N3[] = {768, 3072};
static const int64_t K3[] = {256, 768, 1280, 3072};  // (256: fp32 at <= 16 K stages; 1280: the LayerNorm consumer at > 16)
static const int PATH3[] = {0, 1, 11};
static const int DACT3[] = {ICAP_ACT_NONE, ICAP_ACT_RELU, ICAP_ACT_GELU_NEW};

static void sweep3(int di, Job& job) {
  const PlanDiag d = diag3(di);
  job.default_diag = di == 0;
  for (int64_t M : M3)
    for (int64_t N : N3)
      for (int64_t K : K3)
        for (int path : PATH3)
          for (int trans = 0; trans <= 1; ++trans)
            for (int in_dtype : {ICAP_F32, ICAP_BF16, ICAP_FP8_MX})
              for (int c_dtype : {ICAP_F32, ICAP_BF16})
                for (int act = ICAP_ACT_NONE; act <= ICAP_ACT_GELU_ERF; ++act)
                  for (int dact : DACT3)
                    for (int ln : {LN_NONE, LN_STATS_OUT, LN_STATS_IN})
                      for (int scratch = 0; scratch <= 1; ++scratch) {
                        icap_gemm_args a = base_args(M, N, K, trans, in_dtype, c_dtype);
                        a.path = path;
                        a.act = act;
                        a.dact = dact;
                        if (dact != ICAP_ACT_NONE) a.dact_src = fake<void>(1u << 24), a.ld_dact = N;
                        if (ln == LN_STATS_OUT) a.ln_stats_out = fake<float>(1u << 26);
                        if (ln == LN_STATS_IN) a.ln_stats_in = fake<const float>(1u << 26), a.ln_wsum = fake<const float>(1u << 27);
                        give_scratch(a, scratch, scratch);
                        run_case(a, job, &d);
                      }
}

int main() {
  const int n1 = sizeof M1 / sizeof *M1, n2 = sizeof M2 / sizeof *M2, n3 = N_DIAG3;
  std::vector<Job> jobs(n1 + n2 + n3);
  std::atomic<int> next{0};
  auto work = [&] {
    for (int j; (j = next++) < n1 + n2 + n3;) {
      if (j < n1) sweep1(M1[j], jobs[j]);
      else if (j < n1 + n2) sweep2(M2[j - n1], jobs[j]);
      else sweep3(j - n1 - n2, jobs[j]);
    }
  };
  unsigned nt = std::thread::hardware_concurrency();
  nt = nt < 1 ? 1 : nt > 16 ? 16 : nt;
  std::vector<std::thread> pool;
  for (unsigned t = 1; t < nt; ++t) pool.emplace_back(work);
  work();
  for (auto& t : pool) t.join();
  // the jobs' hashes in job order: the result does not depend on the thread count
  Fnv pinned, all, diag;
  int64_t n_pinned = 0, n_all = 0, n_skipped = 0, n_diag = 0;
  std::vector<unsigned char> planned(N_SLOTS, 0);
  for (int i = 0; i < n1 + n2 + n3; ++i) {
    const Job& j = jobs[i];
    if (i < n1 + n2) {
      pinned.i64((int64_t)j.pinned.h);
      all.i64((int64_t)j.all.h);
    } else {
      diag.i64((int64_t)j.diag.h);
    }
    n_pinned += j.n_pinned, n_all += j.n_all, n_skipped += j.n_skipped, n_diag += j.n_diag;
    for (int k = 0; k < N_SLOTS; ++k) planned[k] |= j.planned[k];
  }
  std::printf("pinned %016llx cases %lld\n", (unsigned long long)pinned.h, (long long)n_pinned);
  if (PLAN_CHECK_ALL_INPUTS) std::printf("all %016llx cases %lld\n", (unsigned long long)all.h, (long long)n_all);
  else std::printf("all skipped: %lld inputs on which these rules divide by zero were not planned\n", (long long)n_skipped);
  std::printf("diag %016llx cases %lld\n", (unsigned long long)diag.h, (long long)n_diag);
  // coverage: every form of the table planned at least once (but the unplannable ones, which stay unplanned)
  int n_forms = 0, n_planned = 0, n_unplannable = 0, n_wrong = 0;
  std::vector<std::string> diag_only;
  for (int k = 0; k < N_SLOTS; ++k) {
    const Form f = form_of_slot(k);
    if (!f.exists()) continue;
    ++n_forms;
    n_planned += planned[k] != 0;
    n_unplannable += unplannable(f);
    if ((planned[k] != 0) == unplannable(f)) {
      ++n_wrong;
      std::printf("%s %s\n", planned[k] ? "planned-unplannable" : "unplanned", form_name(f).c_str());
    }
    if (planned[k] == PLANNED) diag_only.push_back(form_name(f));
  }
  std::printf("forms %d planned %d unplannable %d\n", n_forms, n_planned, n_unplannable);
  for (const std::string& n : diag_only) std::printf("diag-only %s\n", n.c_str());
  return n_wrong == 0 ? 0 : 1;
}
