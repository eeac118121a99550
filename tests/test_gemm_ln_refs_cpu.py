"""The LayerNorm-in-GEMM references, bounds and case list on their own (tests/gemm_ln_refs.py), without a GPU: every
case plans to the kernel instantiation it names, the LayerNorm kinds of the list are those of the table of forms, a plain
fp32 evaluation of every case sits inside the bounds, and every deliberately wrong evaluation exceeds them in every case
it applies to."""

import json
import os

import pytest
import torch

import gemm_epi_refs as R
import gemm_ln_refs as G
from gemm_ln_refs import CASES, LNF, LNS, bf, f32
from gemm_plan_cases import plan
from icap import _lib as L

FORMS_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_kernel_forms.json")
_GN, _QG = R.ACTS["gelu_new"], R.ACTS["quick_gelu"]


@pytest.fixture(scope="module")
def lib():
    return L.load()


def restate(c, wrong=None):
    """(stored outputs, operands) of the case's plain fp32 evaluation; a chain runs its (right) producer's first."""
    if c.form != "chain":
        return G.stored(c, G.evaluate(c, f32, wrong)), None
    p = c.producer()
    first = G.stored(p, G.evaluate(p, f32))
    assert max(G.check(p, first).values()) <= 1.0
    x = G.chain_inputs(c, first["C"], first["stats"])
    return G.stored(c, G.evaluate(c, f32, wrong, x)), x


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_case_plans_to_its_kernel(lib, c):
    name, splits, fused = plan(lib, G.plan_args(c))
    assert name == c.kernel(), (name, c.kernel())
    if c.family == "v0_split":
        assert fused == 1 and splits > 1  # the producer's in-launch split with tickets
    else:
        assert splits == 1
    if c.form == "chain":
        pname, psplits, _ = plan(lib, G.plan_args(c.producer()))
        assert G._kind_of(pname) == LNS and psplits == 1, pname


def test_consumer_never_splits(lib):
    """No admissible consumer shape (K <= 1280: 20 K stages) reaches the in-launch split's 24 stages."""
    for fam in ("v0", "v4"):
        c = G.Case("consumer", fam, (200, 132, 1280), kind=LNF)
        c.kw = {}  # the automatic path with workspace and tickets
        assert plan(lib, G.plan_args(c))[1] == 1


def test_kinds_match_the_table():
    """The LayerNorm kinds the list took from the planner are the table's: the built forms with an LN kind, less
    variant 5 (diagnostic build only) and the 8-phase kernel's fp32-C forms (ln_stats_* requires a bf16 C)."""
    built = [n for n in json.load(open(FORMS_JSON)) if G._kind_of(n) >= LNS]
    v5 = [n for n in built if ", 1, 4, 2, 2, 4, 4, false," in n]
    wide = [n for n in built if n.startswith("icap::gemm8p_kernel<float")]
    assert (len(built), len(v5), len(wide)) == (44, 3, 6)
    table = sorted(set(built) - set(v5) - set(wide))
    first = CASES[:len(G.KINDS)]
    assert sorted(c.kernel() for c in first) == table
    prod = sorted(c.family for c in first if c.form == "producer")
    assert prod == sorted(["v0", "v4", "v12", "v13", "v22", "v24", "v25", "v26", "v27", "v28", "v32", "g8p128", "g8p256"])
    cons = [c for c in first if c.form == "consumer"]
    assert (len(prod), len(cons)) == (13, 22)
    by = lambda k: sorted(c.family for c in cons if c.kind == k)  # noqa: E731
    assert by(LNF) == sorted(["v0", "v4", "v12", "v13", "v22", "v26", "v28", "g8p128", "g8p256"])
    assert by(LNF + R.ACT_FWD + _GN) == sorted(["v0", "v4", "v22", "v26", "v28", "g8p128", "g8p256"])
    assert by(LNF + R.ACT_FWD + _QG) == sorted(["v4", "v22", "v26", "v28"])
    assert by(LNF + R.ACT_ANY) == ["v12", "v13"]
    # the further cases the list promises
    fams = {c.family for c in cons}
    assert {c.family for c in CASES if c.form == "chain"} == fams
    for fam in fams:
        ks = {c.K for c in CASES if c.family == fam and c.form == "consumer"}
        assert ks & {128, 384, 1280} == ks and len(ks) >= (1 if fam == "v0" else 2), (fam, ks)
    for fam in ("v22", "v26", "v28", "g8p128", "g8p256"):
        assert {c.K for c in CASES if c.family == fam and c.form == "consumer"} == {128, 384, 1280}
    sk = [c for c in CASES if c.family == "skinny"]
    assert {(c.form, c.in_dt, c.c_dt, bool(c.act)) for c in sk if c.K == 200} == {
        (f, i, o, a) for f in ("fold", "fused") for i, o in ((bf, bf), (bf, f32), (f32, f32)) for a in (False, True)}
    assert {(c.form, c.K) for c in sk if c.K != 200} == {("fold", 1600), ("fused", 1600)}
    lay = [c for c in CASES if c.m_dev]
    assert {(c.family, c.form, c.live == c.M - 3, c.layout.name) for c in lay} == {
        (f, form, full, "ld%8" if full else "ld=N+1") for f in ("v4", "v26") for form in ("producer", "consumer")
        for full in (True, False)}
    assert all(c.live == 37 for c in lay if c.live != c.M - 3)
    for c in CASES:  # shapes: a partial row tile everywhere; producers N % 32 == 0; consumers K % 128 == 0
        assert c.M % 32 and (c.form != "producer" or c.N % 32 == 0) and (not c.rows_out or c.K % 128 == 0)


def test_planted_inputs():
    x = G.ln_inputs(bf, bf, 300, 264, 384)
    mean, M2 = G.combine(x.stats, torch.float64)
    rstd = G.rstd_of(M2, 384, G.EPS)
    assert M2[0] == 0 and M2[1] == 0 and mean[1] == 300 and abs(rstd[0] - G.EPS ** -0.5) < 1e-9
    assert abs(mean[2] - 300) < 1 and 1 < (M2[2] / 384).sqrt() < 2 and abs((M2[3] / 384).sqrt() - 0.348) < 1e-3
    within = x.stats[:, :, 1].double().sum(-1)
    assert within[4] == 384 * 0.25 and M2[4] > 50 * within[4] and within[5] == within[4] and M2[5] > 50 * within[5]
    assert not x.stats[6, :, 0].any() and x.stats[6, :, 1].max() == 64 * x.stats[6, :, 1].min()
    assert M2[8] / 384 < G.EPS and M2[7] / 384 < G.EPS
    p = G.prod_inputs(300, 288, 200)
    C = G.evaluate(G.Case("producer", "v26", (300, 288, 200), kind=LNS))["C"]
    assert torch.equal(C[16:24, :64], p.resid[16:24, :64].double())  # exact: A = 0, bias = 0 there
    st = G.group_stats(C[16:20, :64])
    assert not st[0, :, 1].any() and st[1, 0, 0] == (31 + 100) / 32 and st[3, 0, 1] == 0 and st[3, 1, 1] == 4 * 31 / 32


WORST = {}


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_plain_fp32_inside_bounds(c):
    got, x = restate(c)
    w = G.check(c, got, x)
    key = c.form + ("" if c.family != "skinny" else f" {R.dt_name(c.in_dt)}/{R.dt_name(c.c_dt)}")
    for k, v in w.items():
        WORST[key, k] = max(WORST.get((key, k), 0.0), v)
    extra = ""
    if c.form == "producer":
        extra = " flips (exact rows, others) %s of %d" % (G.flips(c, got["C"]), got["C"].numel())
    if c.form == "fused" and c.in_dt == bf:
        extra = " boundary share (all rows, random rows) %.4f %.4f" % G.boundary_share(c)
    print(f"{c.name}: plain fp32 worst ratios " + " ".join(f"{k} {v:.3f}" for k, v in w.items()) + extra)
    assert max(w.values()) <= 1.0, w


def test_plain_fp32_summary():
    """(prints the per-form maxima of the test above when it ran in the same session)"""
    for (form, k), v in sorted(WORST.items()):
        print(f"{form:16s} {k:7s} {v:.3f}")


# wrong evaluation -> the cases it applies to (every one of them must exceed its bound). A chain's A is whatever its
# producer stored: it has no planted rows, so what only those show (eps, the one-pass cancellation) is left to the
# consumer cases of the same kernels, and a faulty producer is the producer cases' to catch (its statistics against
# the C it stored); a chain sees every fault of the combine and of the fold.
_planted = ("consumer", "fold", "fused")
APPLIES = {
    # an fp32 E x^2 - mean^2 on bf16 data (offset / spread <= 2^8) errs by about the rounding of a bf16 C, and in the
    # fold by less than rstd dacc, which grows with the offset too: it shows in ln_rstd_out, in the fused form through
    # an fp32 C (not at K = 1600 in bf16, where the two-pass loop's own budget of 105 adds is as wide), in the fold on
    # fp32 rows (planted row 10). (The skinny kernel's short bf16 rows ARE taken in one pass, over x - x0.)
    "onepass": lambda c: (c.form == "consumer" or (c.form == "fused" and c.c_dt == f32 and (c.frag or c.in_dt == f32)) or
                          (c.form == "fold" and c.in_dt == f32)),
    "no_between": lambda c: c.rows_out,
    "n31": lambda c: c.rows_out or c.form == "producer",
    "n33": lambda c: c.rows_out or c.form == "producer",
    "k_minus_1": lambda c: c.form != "producer",
    "eps_outside": lambda c: c.form in _planted,
    "no_eps": lambda c: c.form in _planted,
    "half_groups": lambda c: c.rows_out,
    "half_mean": lambda c: c.rows_out,
    "scale_acc_only": lambda c: c.form in ("consumer", "chain", "fold"),
    "bias_inside": lambda c: c.form in ("consumer", "chain", "fold"),
    "act_first": lambda c: c.form in ("consumer", "chain", "fold") and c.act,
    "unrounded": lambda c: c.form == "producer",
    "before_resid": lambda c: c.form == "producer",
    "shift8": lambda c: c.form == "producer",
    "miss_lane": lambda c: c.form == "producer",
    # rounding a or not moves the product by about 2^-9 |a| |b| sqrt K: below the rounding of a bf16 C, so an fp32 C
    "a_unrounded": lambda c: c.form == "fused" and c.in_dt == bf and c.c_dt == f32,
}


@pytest.mark.parametrize("wrong", sorted(APPLIES))
def test_wrong_evaluation_exceeds_bound(wrong):
    cases = [c for c in CASES if APPLIES[wrong](c)]
    assert cases
    low = {}
    for c in cases:
        got, x = restate(c, wrong)
        w = max(G.check(c, got, x).values())
        if not w > 1.0:
            low[c.name] = w
    print(f"{wrong}: {len(cases)} cases")
    assert not low, low
