"""The LayerNorm backward's fp64 reference, cases and bounds (tests/ln_bwd_refs.py) checked without a GPU: the
formula against torch.autograd in fp64, every bound against a plain fp32 evaluation of the formula (the bound is
attainable, and that evaluation fixes the constants) and against a list of deliberately wrong results (the bound
notices each by a wide margin), the case list against a restatement of the dispatch."""

import math

import pytest
import torch

import ln_bwd_refs as R

bf, f32 = torch.bfloat16, torch.float32
BOTH = (bf, f32)
WIDE_MARGIN = 50.0      # what "exceeds its bound by a wide margin" asks of every wrong result below


# ------------------------------------------------------------------------------------------------ the case list


def test_cases_reach_every_instantiation():
    names = {c.reaches for c in R.CASES}
    want = {f"ln_bwd8_kernel<{dt}, {p}, {k}>" for dt in ("bf16", "f32") for p in ("true", "false")
            for k in (3, 4, 5, 6)} | {"ln_bwd_kernel<bf16>", "ln_bwd_kernel<f32>"}
    assert names == want
    assert len({c.name for c in R.CASES}) == len(R.CASES)
    for c in R.CASES + R.BATCH_CASES:
        assert c.D % 4 == 0 and all(s % 4 == 0 and s >= c.D for s in (c.ldx, c.lddy, c.lddres, c.lddx))
        assert c.D <= 1024 or c.reaches.startswith("ln_bwd8")
        assert c.rows * max(c.ldx, c.lddx) <= 2.2e6          # a few thousand to about 2 M elements
        es = 2 if c.dtype == bf else 4
        assert (c.x_off * es) % 8 == 0                       # the 4-wide kernel's accesses stay aligned
    # the 4-wide kernel with and without parameters, dres, a row map, rows_dev and dx_drop; the same for the 8-wide
    for k in ("ln_bwd_kernel<", "ln_bwd8_kernel<"):
        fam = [c for c in R.CASES if c.reaches.startswith(k)]
        for prop in (lambda c: c.params, lambda c: not c.params, lambda c: not c.dres, lambda c: c.rowmap,
                     lambda c: c.rows_dev is not None, lambda c: c.drop_p > 0, lambda c: c.accumulate,
                     lambda c: c.dgamma and not c.dbeta, lambda c: c.dbeta and not c.dgamma,
                     lambda c: c.lddx > c.D, lambda c: c.lddy > c.D, lambda c: c.dres and c.lddres > c.D):
            assert any(prop(c) for c in fam)
    # each single stride at 772 and the bf16 base 8 bytes in send a D = 768 call to the 4-wide kernel
    for dt in BOTH:
        for k in ("ldx", "lddy", "lddres", "lddx"):
            assert R._c(9, 768, dt, **{k: 772}).reaches.startswith("ln_bwd_kernel<")
            assert R._c(9, 768, dt, **{k: 776}).reaches.startswith("ln_bwd8_kernel<")
    assert R._c(9, 768, bf, x_off=4).reaches == "ln_bwd_kernel<bf16>"
    assert R._c(9, 768, f32, x_off=4).reaches == "ln_bwd8_kernel<f32, true, 3>"
    assert R._c(9, 768, f32, lddres=772, dres=False).reaches.startswith("ln_bwd8")   # an absent dres does not count


def test_launch_shapes():
    """(blocks, rows per pass, passes, blocks without a row), restated from icap_layernorm_bwd."""
    by = {c.name: c for c in R.CASES}
    assert R.launch(by["12x768-bf16"]) == (3, 24, 1, 1)         # the 8-wide form on the 4-wide form's block count
    assert R.launch(by["37x768-bf16"]) == (10, 80, 1, 5)
    assert R.launch(by["12x132-f32"]) == (3, 12, 1, 0)
    assert R.launch(by["2057x64-bf16"]) == (256, 2048, 2, 0)    # second pass: 9 rows
    assert R.launch(by["1029x36-f32"]) == (256, 1024, 2, 0)     # 5 rows, each prefetched during the first pass
    assert R.launch(by["32777x64-f32-nodgamma-nodbeta"]) == (4096, 32768, 2, 0)
    assert R.launch(by["16389x36-bf16-nodgamma-nodbeta"]) == (4096, 16384, 2, 0)
    assert R.launch(by["37x768-bf16-live0"]) == (10, 80, 0, 10)
    assert R.launch(by["9x768-f32-nodgamma-nodbeta"]) == (2, 16, 1, 0)
    for name in ("2057x64", "1029x36"):
        for dt in ("bf16", "f32"):
            assert by[f"{name}-{dt}-rowmap-accumulate"].rowmap
    assert [R.launch(c)[0] for c in R.BATCH_CASES] == [10, 3, 256]
    assert [c.D for c in R.BATCH_CASES] == [768, 132, 64]
    assert [(c.accumulate, c.dgamma, c.dbeta) for c in R.BATCH_CASES] == [(True, True, True), (False, True, True),
                                                                         (False, True, False)]


def test_rejected_calls_break_a_requirement():
    assert all(not R.accepted(r) for r in R.REJECTED)
    assert R.accepted(R.Rejected("fine", 768)) and R.accepted(R.Rejected("fine", 1032, lddx=1040))
    assert R.accepted(R.Rejected("fine", 768, lddy=772)) and R.accepted(R.Rejected("fine", 1020))
    whys = {r.why for r in R.REJECTED}
    assert {"D 6", "D 1028", "D 1544", "D 1032 lddx 1036", "no workspace", "drop_p 1"} <= whys
    for k in ("ldx", "lddy", "lddres", "lddx"):   # a stride that is no multiple of 4 on each operand, both forms
        assert {f"{k} 770", f"{k} 134"} <= whys


def test_inputs_poison_what_must_not_be_read():
    for c in R.CASES:
        if c.rows > 2057:
            continue
        t = c.inputs()
        n = c.live
        assert torch.isnan(t["x"][n:]).all() and torch.isfinite(t["x"][:n]).all()
        assert torch.isnan(t["mean"][n:]).all() and torch.isnan(t["rstd"][n:]).all()
        if c.dres:
            assert torch.isnan(t["dres"][n:]).all() and torch.isfinite(t["dres"][:n]).all()
        g = t["gather"]
        used = set(g[g >= 0].tolist())
        for r in range(min(c.rows, 64)):
            assert bool(torch.isnan(t["dy"][r]).all()) == (r not in used)
        if c.rowmap and n:
            assert int((g < 0).sum()) == (n + 3) // 4 and len(used) == n - (n + 3) // 4
        ref = R.reference(c)
        assert all(torch.isfinite(ref[k]).all() for k in ("dx", "dgamma", "dbeta", "A_dx"))
        assert ref["dx"].shape == (n, c.D)
    # ln_bwd8_kernel reads dy row 0 for a negative map entry and selects afterwards: in some case that row is NaN
    assert any(c.rowmap and c.reaches.startswith("ln_bwd8") and torch.isnan(c.inputs()["dy"][0]).all()
               for c in R.CASES)


# ------------------------------------------------------------------------------------------------ the reference


@pytest.mark.parametrize("case", [c for c in R.CASES if c.rows <= 37 and c.live > 0], ids=repr)
def test_formula_matches_autograd(case):
    """With the row statistics in fp64 (not the fp32-rounded ones the kernel is handed) the formula is
    torch.autograd's gradient of layer_norm to 1e-12."""
    t = case.inputs()
    n, D = case.live, case.D
    x = t["x"][:n].double().requires_grad_(True)
    g = t["gamma"].double().requires_grad_(True)
    b = torch.zeros(D, dtype=torch.float64, requires_grad=True)
    dyp = R.gathered_dy(t, n)
    y = torch.nn.functional.layer_norm(x, (D,), g, b, R.f32r(R.LN_EPS))
    gx, gg, gb = torch.autograd.grad(y, (x, g, b), dyp)
    xd = x.detach()
    mean = xd.mean(1)
    rstd = 1.0 / torch.sqrt(((xd - mean[:, None]) ** 2).mean(1) + R.f32r(R.LN_EPS))
    dres = None if t["dres"] is None else t["dres"][:n].double()
    r = R.formula(xd, g.detach(), mean, rstd, dyp, dres)
    assert torch.allclose(r["dx"] - (0 if dres is None else dres), gx, rtol=1e-12, atol=1e-12)
    assert torch.allclose(r["dgamma"], gg, rtol=1e-12, atol=1e-12)
    assert torch.allclose(r["dbeta"], gb, rtol=1e-12, atol=1e-12)
    # and the reference proper (fp32-rounded statistics) is that gradient up to the statistics' rounding
    ref = R.reference(case)
    init = t["dgamma0"].double() if case.accumulate else 0.0
    assert torch.allclose(ref["dx"], r["dx"], rtol=0, atol=1e-5 * ref["A_dx"].max().item())
    assert torch.allclose(ref["dgamma"] - init, gg, rtol=0, atol=1e-5 * ref["A_dgamma"].max().item())


def test_rowmap_cases_are_among_the_autograd_checks():
    seen = [c for c in R.CASES if c.rows <= 37 and c.live > 0]
    assert any(c.rowmap for c in seen) and any(not c.rowmap for c in seen)
    assert any(c.rowmap and c.rows_dev is not None for c in seen)


# ------------------------------------------------------------------------------------------------ the bounds


@pytest.mark.parametrize("case", R.CASES + R.BATCH_CASES, ids=repr)
def test_bounds_hold_for_an_fp32_evaluation(case):
    got = R.ln_bwd_fp32(case)
    ratios = (R.dx_ratio(case, got["dx"]),) + R.param_ratios(case, got["dgamma"] if case.dgamma else None,
                                                             got["dbeta"] if case.dbeta else None)
    print(case, "fp32 evaluation, error / bound (dx, dgamma, dbeta):", ratios)
    assert max(ratios) <= 1.0
    assert R.untouched(case, R.layout(case, got["dx"]))
    if case.drop_p > 0:
        keep = case.keep()[:case.live]
        dxd = (R.ln_bwd_fp32(case, rounded=False)["dx"] * keep * torch.tensor(R.inv_keep(case.drop_p), dtype=f32))
        assert R.dx_drop_ratio(case, dxd.to(case.dtype)) <= 1.0
        assert 0.05 < 1 - keep.double().mean().item() < 0.15


def test_constants_follow_the_fp32_measurement():
    """K_DX and K_P are the next power of two at or above 4 x the worst ratio of the fp32 evaluation with K = 1
    (measured on the fp32 value before a bf16 case's rounding), over all cases."""
    dx = g = b = 0.0
    for c in R.CASES + R.BATCH_CASES:
        got = R.ln_bwd_fp32(c, rounded=False)
        dx = max(dx, R.dx_ratio(c, got["dx"], k=1.0, r16=0.0))
        pg, pb = R.param_ratios(c, got["dgamma"] if c.dgamma else None, got["dbeta"] if c.dbeta else None, k=1.0)
        g, b = max(g, pg), max(b, pb)
    print(f"fp32 evaluation, error / (U * A): dx {dx:.3g}, dgamma {g:.3g}, dbeta {b:.3g}")
    assert R.K_DX == 2.0 ** math.ceil(math.log2(4 * dx))
    assert R.K_P == 2.0 ** math.ceil(math.log2(4 * max(g, b)))


# ------------------------------------------------------------------------------------------------ wrong results


def pieces(case):
    """fp64 x, gamma, mean, rstd, dy (ungathered), dres, map of ALL rows from the unpoisoned inputs (the statistics
    of the dead rows computed like the live ones'), for building wrong results that read what they must not."""
    t = case.base().inputs()
    x = t["x"].double()
    mean = x.mean(1)
    rstd = 1.0 / torch.sqrt(((x - mean[:, None]) ** 2).mean(1) + R.f32r(R.LN_EPS))
    live = case.inputs()
    mean[:case.live], rstd[:case.live] = live["mean"][:case.live].double(), live["rstd"][:case.live].double()
    rm = torch.arange(case.rows) if t["rowmap"] is None else t["rowmap"].long()
    return dict(x=x, gamma=t["gamma"].double(), mean=mean, rstd=rstd, dy=t["dy"].double(),
                dres=None if t["dres"] is None else t["dres"].double(), rm=rm)


def gather(p, rm):
    return torch.where((rm >= 0)[:, None], p["dy"][rm.clamp_min(0)], torch.zeros_like(p["dy"]))


def right(case, p):
    return R.formula(p["x"], p["gamma"], p["mean"], p["rstd"], gather(p, p["rm"]), p["dres"])


def stored(case, dx):
    """What a kernel would store of fp64 `dx`: the live rows in the case's dtype."""
    return dx[:case.live].to(case.dtype)


@pytest.mark.parametrize("dt", BOTH, ids=R.dt_name)
def test_wrong_dx_is_noticed(dt):
    case = R._c(37, 768, dt)
    p = pieces(case)
    ok = right(case, p)
    assert R.dx_ratio(case, stored(case, ok["dx"])) <= 1.0      # the rounded reference itself passes
    xh = (p["x"] - p["mean"][:, None]) * p["rstd"][:, None]
    gy = p["dy"] * p["gamma"]
    m1, m2 = gy.mean(1, keepdim=True), (gy * xh).mean(1, keepdim=True)
    rs = p["rstd"][:, None]
    row = 5
    wrong = {
        "one row without xh * m2": rs * (gy - m1) + p["dres"],
        "one row without m1": rs * (gy - xh * m2) + p["dres"],
        "dres missing in one row": rs * (gy - m1 - xh * m2),
    }
    seen = {}
    for name, w in wrong.items():
        dx = ok["dx"].clone()
        dx[row] = w[row]
        seen[name] = R.dx_ratio(case, stored(case, dx))
    shifted = dict(p, mean=p["mean"].roll(1), rstd=p["rstd"].roll(1))
    seen["mean / rstd shifted by one row"] = R.dx_ratio(case, stored(case, right(case, shifted)["dx"]))
    print(R.dt_name(dt), {k: float(f"{v:.3g}") for k, v in seen.items()})
    assert min(seen.values()) > WIDE_MARGIN, seen
    if dt == bf:
        assert seen["one row without xh * m2"] >= 200.0
    # what the max-norm check of test_kernels_gpu.py test_layernorm (2e-2 for bf16) lets through
    dx = ok["dx"].clone()
    dx[row] = wrong["one row without m1"][row]
    old = ((dx - ok["dx"]).abs().max() / ok["dx"].abs().max()).item()
    print(f"one row without m1: max-norm error {old:.3g}")
    assert old < 2e-2


@pytest.mark.parametrize("dt", BOTH, ids=R.dt_name)
def test_wrong_rowmap_is_noticed(dt):
    case = R._c(37, 132, dt, rowmap=True)
    p = pieces(case)
    assert R.dx_ratio(case, stored(case, right(case, p)["dx"])) <= 1.0
    rm = p["rm"]
    assert int((rm < 0).sum()) == 10 and int(rm[0]) < 0
    seen = {}
    for name, m in (("dy from row r", torch.arange(case.rows)), ("a negative entry given row 0's dy", rm.clamp_min(0))):
        r = R.formula(p["x"], p["gamma"], p["mean"], p["rstd"], gather(p, m), p["dres"])
        seen[name] = (R.dx_ratio(case, stored(case, r["dx"])),) + R.param_ratios(case, r["dgamma"], r["dbeta"])
    print(R.dt_name(dt), seen)
    assert all(min(v) > WIDE_MARGIN for v in seen.values()), seen


@pytest.mark.parametrize("dt", BOTH, ids=R.dt_name)
def test_wrong_parameter_sums_are_noticed(dt):
    seen = {}

    def contributions(case):
        p = pieces(case)
        dyp = gather(p, p["rm"])
        xh = (p["x"] - p["mean"][:, None]) * p["rstd"][:, None]
        init = case.inputs()
        g0 = init["dgamma0"].double() if case.accumulate else 0.0
        b0 = init["dbeta0"].double() if case.accumulate else 0.0
        return dyp * xh, dyp, g0, b0

    for case in (R._c(37, 768, dt), R._c(2057, 64, dt)):
        cg, cb, _, _ = contributions(case)
        n = case.live
        assert max(R.param_ratios(case, cg.sum(0), cb.sum(0))) <= 1.0
        nb, per_pass, passes, _ = R.launch(case)
        sums = {"without the last live row": slice(0, n - 1), "without the odd rows (one half-wave)": slice(0, n, 2)}
        if passes == 2:
            sums["without the second pass's rows"] = slice(0, per_pass)
        for name, s in sums.items():
            seen[f"{case}: {name}"] = R.param_ratios(case, cg[s].sum(0), cb[s].sum(0))
    big = seen[f"{R._c(2057, 64, dt)}: without the last live row"]
    assert min(big) >= 500.0
    case = R._c(37, 768, dt, live=29)
    cg, cb, _, _ = contributions(case)
    assert max(R.param_ratios(case, cg[:29].sum(0), cb[:29].sum(0))) <= 1.0
    seen["one row past live"] = R.param_ratios(case, cg[:30].sum(0), cb[:30].sum(0))
    case = R._c(37, 768, dt, accumulate=True)
    cg, cb, g0, b0 = contributions(case)
    assert max(R.param_ratios(case, g0 + cg.sum(0), b0 + cb.sum(0))) <= 1.0
    seen["accumulate treated as overwrite"] = R.param_ratios(case, cg.sum(0), cb.sum(0))
    case = R._c(37, 768, dt)
    other = R._c(37, 768, dt, accumulate=True).inputs()
    seen["overwrite treated as accumulate"] = R.param_ratios(case, other["dgamma0"].double() + cg.sum(0),
                                                             other["dbeta0"].double() + cb.sum(0))
    print(R.dt_name(dt), {k: tuple(float(f"{x:.3g}") for x in v) for k, v in seen.items()})
    assert all(min(v) > WIDE_MARGIN for v in seen.values()), seen


def test_dead_call_must_leave_exact_zeros():
    case = next(c for c in R.CASES if c.rows_dev == 0 and c.params)
    z = torch.zeros(case.D)
    assert R.param_ratios(case, z, z) == (0.0, 0.0)
    assert R.param_ratios(case, z + 1e-30, z)[0] == math.inf
    assert R.param_ratios(case, torch.full((case.D,), float("nan")), z)[0] == math.inf   # an unwritten gradient
    assert R.dx_ratio(case, torch.full((case.rows, case.lddx), R.SENTINEL)) == 0.0


def test_nan_in_a_result_is_an_infinite_ratio():
    case = R._c(9, 768, bf)
    dx = R.ln_bwd_fp32(case)["dx"].clone()
    dx[3, 5] = float("nan")
    assert R.dx_ratio(case, dx) == math.inf


def test_wrong_dx_drop_is_noticed():
    case = next(c for c in R.CASES if c.drop_p > 0 and c.lddx > c.D and c.dtype == f32)
    ref = R.reference(case)
    assert R.dx_drop_ratio(case, ref["dx_drop"].float()) <= 1.0
    assert R.dx_drop_ratio(case, (ref["dx"] * R.inv_keep(case.drop_p)).float()) == math.inf   # nothing dropped
    ld = R.site_keep(R.make_desc(case.drop_p, case.big)[0], (case.rows, case.lddx),
                     R.make_desc(case.drop_p, case.big)[1])[:, :case.D]      # the mask indexed with the stride
    assert R.dx_drop_ratio(case, (ref["dx"] * ld * R.inv_keep(case.drop_p)).float()) == math.inf


# ------------------------------------------------------------------------------------------------ the layout check


def test_layout_check_flags_each_kind_of_damage():
    case = next(c for c in R.CASES if c.lddx > c.D and c.rows_dev is None)
    live = next(c for c in R.CASES if c.rows_dev == 29)
    for c in (case, live):
        good = R.layout(c, R.ln_bwd_fp32(c)["dx"])
        assert good.shape == (c.rows, c.lddx) and R.untouched(c, good)
        bad = good.clone()
        bad[2, 7] = R.SENTINEL            # a live element the kernel did not write
        assert not R.untouched(c, bad)
    bad = R.layout(case, R.ln_bwd_fp32(case)["dx"])
    bad[4, case.D] = 0.0                  # the first padding element of a row
    assert not R.untouched(case, bad)
    bad = R.layout(live, R.ln_bwd_fp32(live)["dx"])
    bad[29, 0] = 0.0                      # the first row past rows_dev
    assert not R.untouched(live, bad)
