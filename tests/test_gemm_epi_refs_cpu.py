"""The GEMM epilogue references, bounds and case list on their own (tests/gemm_epi_refs.py), without a GPU: every case
plans to the kernel instantiation it names, the list reaches the coverage it claims, a plain fp32 evaluation of every
case sits inside the bounds, every deliberately wrong epilogue exceeds them in every (in dtype, C dtype) set, and the
validator rejects what it documents."""

import ctypes as C

import pytest
import torch

import gemm_epi_refs as R
from gemm_epi_refs import ACTS, CASES, Case, bf, f32
from gemm_plan_cases import gemm_args, plan
from icap import _lib as L

SETS = [(f32, f32), (bf, bf), (bf, f32), (f32, bf)]
_GN, _QG, _RELU, _ERF, _TANH = (ACTS[k] for k in ("gelu_new", "quick_gelu", "relu", "gelu_erf", "tanh"))


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _round(c, C_, aux):
    return C_.to(c.c_dt), None if aux is None else aux.to(c.c_dt)


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_case_plans_to_its_kernel(lib, c):
    name, splits, fused = plan(lib, R.plan_args(c))
    assert name == c.kernel(), (name, c.kernel())
    if c.family == "v0":
        assert fused == 1 and splits > 1  # the in-launch split with tickets
    elif c.family == "reduce":
        assert fused == 0 and splits > 1
    else:
        assert splits == 1


def test_coverage():
    have = {(c.family, c.act, c.dact, c.c_dt, c.kind) for c in CASES if c.in_dt == bf and c.layout is R.PLAIN}
    # the 23 specialised kinds with a bf16 C; with an fp32 C the 4 the table has (8-phase), the other 19 pinned to
    # the dispatching kind they plan to
    n_spec = n_any = 0
    for fam, kinds in R.SPECIALISED.items():
        for a, d in kinds:
            assert (fam, a, d, bf, "spec") in have, (fam, a, d)
            n_spec += 1
            if fam in R.F32_C_SPECIALISED:
                assert (fam, a, d, f32, "spec") in have, (fam, a, d)
                n_spec += 1
            else:
                assert (fam, a, d, f32, "any") in have, (fam, a, d)
                n_any += 1
    assert (n_spec, n_any) == (23 + 4, 19)
    assert sorted((f, len(k)) for f, k in R.SPECIALISED.items()) == [
        ("g8p128", 2), ("g8p256", 2), ("v0", 2), ("v13", 2), ("v22", 3), ("v26", 3), ("v28", 5), ("v4", 4)]
    # a specialised case names a specialised instantiation (ACT integer 16 + a / 32 + a), a dispatching one 1
    for c in CASES:
        if c.kind == "spec":
            assert c.actk() in (16 + c.act, 32 + c.dact) and f", {c.actk()}" in c.kernel()
    # base tile path and skinny kernel: all five activations both ways, fp32 in / fp32 C
    for fam in ("v4_f32in", "skinny"):
        for a in ACTS.values():
            assert any(c.family == fam and c.in_dt == f32 and c.c_dt == f32 and c.act == a for c in CASES)
            assert any(c.family == fam and c.in_dt == f32 and c.c_dt == f32 and c.dact == a for c in CASES)
    # the dispatching kind on every family: tanh forward and a derivative the family does not specialise
    fams = set(R.DISPATCH_FAMILIES)
    assert {"v12", "v16", "v24", "v25", "v27", "v32", "v14", "v15", "v31", "g256", "reduce", "skinny"} <= fams
    for fam in fams:
        assert any(c.family == fam and c.kind == "any" and c.act == _TANH for c in CASES), fam
        assert any(c.family == fam and c.kind == "any" and c.dact and (0, c.dact) not in R.SPECIALISED.get(fam, [])
                   for c in CASES), fam
    # the layout axes on the base tile path and a ring family
    for fam in ("v4", "v26_n130"):
        lay = [c for c in CASES if c.family == fam and c.layout is not R.PLAIN]
        assert all(c.m_dev and c.live == c.M - 3 and c.N == 130 for c in lay)
        assert {c.layout.name for c in lay} == {"ld%8", "ld=N+1", "off1"}
        assert {c.beta for c in lay if c.act} == {0.0, 0.5, 1.0} == {c.beta for c in lay if c.dact}
        assert all(c.c_dt == f32 for c in lay if c.beta)
        for c in lay:
            ldc, ldaux, ldr, ldd = c.lds()
            if c.layout.name == "ld%8":
                assert len({ldc, ldaux, ldr, ldd}) == 4 and all(v % 8 == 0 for v in (ldc, ldaux, ldr, ldd))
            if c.layout.name == "ld=N+1":
                assert ldc == c.N + 1
            assert c.N + c.layout.off <= min(ldc, ldaux, ldr, ldd)


def test_grid_and_inputs():
    g = torch.tensor(R.GRID, dtype=torch.float64)
    assert torch.equal(g.to(bf).double(), g) and torch.equal((2 * g).to(bf).double(), 2 * g)
    assert g.abs().max() == 12 and len(set(R.GRID)) == len(R.GRID) - 1  # (+0 and -0 compare equal)
    for in_dt, c_dt in SETS:
        x = R.inputs(in_dt, c_dt, 100, 130, 200)
        z = 0.5 * x.acc[:R.P]
        free = x.bias == 0
        # every grid value reaches a bias-free column of a planted row, as z and as dact_src
        assert set(z[:, free].flatten().tolist()) == set(R.GRID)
        assert set(R.GRID) <= set(x.dsrc[:R.P // 2].double().flatten().tolist())
        assert free.sum() >= 60 and (~free).sum() >= 60
        if c_dt == f32:
            s = x.dsrc[R.P // 2:R.P]
            assert (s.to(bf).float() != s).any()


def test_lipschitz_constants():
    z = torch.linspace(-14, 14, 560001, dtype=torch.float64)
    for a in (_GN, _QG, _ERF):
        sup = R.dact_ref(a, z).abs().max().item()
        assert sup <= R.L_ACT[a] < sup + 0.04, (a, sup)
    assert R.dact_ref(_TANH, torch.tanh(z)).abs().max() <= 1 and R.L_ACT[_RELU] == 1


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_plain_fp32_inside_bounds(c):
    w = R.check(c, *_round(c, *R.evaluate(c, f32)))
    print(f"{c.name}: plain fp32 worst ratio {w:.3f}")
    assert w <= 1.0, w


# (wrong variant, forward activation, backward activation): the launches in which it must show
WRONG = [("swap_gelus", _ERF, 0), ("swap_gelus", _GN, 0), ("swap_gelus", 0, _ERF), ("swap_gelus", 0, _GN),
         ("quick_1.7", _QG, 0), ("quick_1.7", 0, _QG), ("gelu_new_cubic", 0, _GN), ("aux_is_act", _GN, 0),
         ("aux_is_act", _RELU, 0), ("aux_is_pre", _TANH, 0), ("alpha_times_sum", _QG, 0), ("bwd_no_alpha", 0, _GN),
         ("relu_at_0", 0, _RELU), ("resid_first", _GN, 0), ("resid_first", _RELU, 0), ("beta_on_v", _GN, 0),
         ("beta_on_v", 0, _GN)]


@pytest.mark.parametrize("wrong,act,dact", WRONG, ids=lambda v: str(v))
@pytest.mark.parametrize("in_dt,c_dt", SETS, ids=R.dt_name)
def test_wrong_variant_exceeds_bound(in_dt, c_dt, wrong, act, dact):
    if wrong == "beta_on_v" and c_dt == bf:
        return  # beta != 0 needs an fp32 C: the variant does not exist for a bf16 C
    fam = "v4" if in_dt == bf else "v4_f32in"
    c = Case(fam, in_dt, c_dt, act=act, dact=dact, beta=0.5 if wrong == "beta_on_v" else 0.0)
    right = R.check(c, *_round(c, *R.evaluate(c)))
    w = R.check(c, *_round(c, *R.evaluate(c, wrong=wrong)))
    print(f"{wrong} {c.name}: right {right:.3f} wrong {w:.3g}")
    assert right <= 1.0 < w, (right, w)


def test_rejections(lib):
    def err(**kw):
        a = gemm_args(200, 128, 64, **kw)
        assert lib.icap_gemm_kernel_name(C.byref(a)) is None
        return plan(lib, a)[0]

    assert err(beta=0.5) == "icap_gemm: beta != 0 requires f32 C"
    a = gemm_args(200, 128, 64, dact=_GN)
    a.dact_src = None
    assert plan(lib, a)[0] == "icap_gemm: dact requires dact_src"
    assert err(act=6) == "icap_gemm: unknown activation"
    assert plan(lib, gemm_args(200, 128, 64, beta=0.5, c_dtype=L.F32))[1] is not None
