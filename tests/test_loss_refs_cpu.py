"""The loss tail's fp64 references, cases and bounds (tests/loss_refs.py) checked without a GPU: each reference
against torch's own fp64 implementation, each bound against a plain fp32 evaluation of the formula (the bound is
attainable) and against a deliberately wrong result (the bound notices)."""

import math

import pytest
import torch

import loss_refs as R

bf, f32 = torch.bfloat16, torch.float32


# ------------------------------------------------------------------------------------------------ cross entropy


def test_ce_cases_reach_the_kernels_their_names_say():
    """csrc/elementwise.hip icap_cross_entropy's dispatch, restated: every kernel is reached, each form at least
    once with dlogits (the GPU test runs every such case out of place and in place)."""
    for c in R.CE_CASES:
        assert c.ld >= c.V and c.ld % 4 == 0 and (c.rows <= 40 or c.rows == 300)
        es = 2 if c.dtype == bf else 4
        assert (c.offset * es) % 8 == 0  # the two-pass kernel's 4-element accesses stay aligned
        reg = c.dtype == bf and c.V <= 8 * 512 * 13 and c.ld % 8 == 0 and (c.offset * es) % 16 == 0
        assert c.reaches == ("ce_bf16_reg_kernel<13>" if reg else
                             "ce_kernel<bf16>" if c.dtype == bf else "ce_kernel<float>"), c
    for k in ("ce_bf16_reg_kernel<13>", "ce_kernel<bf16>", "ce_kernel<float>"):
        assert any(c.reaches == k and c.dlogits for c in R.CE_CASES)
        assert any(c.reaches == k and c.rows_dev for c in R.CE_CASES) or k == "ce_kernel<bf16>"


def test_ce_labels_cover_the_edges():
    c = R.CE_CASES[0]
    y = c.labels().tolist()
    assert c.V % 8 == 1 and c.V - 1 in y  # the label in the V % 8 tail
    assert all(v in y for v in (0, 4095, 4096, 1000, 1001))
    assert y[0] == -100 and y[-1] == -100 and y[10:13] == [-100] * 3
    for c in R.CE_CASES:
        y = c.labels()
        assert y[0] == -100 and y[c.live - 1] == -100 and int((y[:c.live] >= 0).sum()) > 0
        assert int(y.max()) < c.V and (c.V - 1 in y.tolist() or c.V == 1)


@pytest.mark.parametrize("case", R.CE_CASES, ids=repr)
def test_ce_reference_matches_torch(case):
    t = case.inputs()
    n, V = case.live, case.V
    x = t["logits"][:n, :V].double().requires_grad_(True)
    y = t["labels"][:n].long()
    loss = torch.nn.functional.cross_entropy(x, y, ignore_index=-100)
    (gx,) = torch.autograd.grad(loss, x)
    ref = R.ce_reference(case)
    assert abs(ref["loss"] - loss.item()) <= 1e-12 * max(1.0, abs(loss.item()))
    d = ref["dlogits"]
    assert torch.allclose(d[:, :V], gx * R.f32r(case.grad_scale), rtol=1e-10, atol=1e-300)
    assert torch.equal(d[:, V:], torch.zeros_like(d[:, V:])) and torch.equal(d[y < 0], torch.zeros_like(d[y < 0]))
    assert torch.equal(ref["loss_rows"][y < 0], torch.zeros(int((y < 0).sum()), dtype=torch.float64))
    # the two special rows: all-equal logits give log V; the 1e4 logit gives a finite loss and an exact one-hot
    assert abs(ref["loss_rows"][7].item() - math.log(V)) < 1e-12
    if V > 1:
        spike = t["logits"][8, :V].double().max().item()
        assert spike > 9e3 and abs(ref["loss_rows"][8].item() - (spike - x[8, y[8]].item())) < 1e-9
        assert torch.isfinite(d[8]).all() and int((d[8] != 0).sum()) == 2


@pytest.mark.parametrize("case", R.CE_CASES, ids=repr)
def test_ce_bounds_hold_for_an_fp32_evaluation(case):
    loss, loss_rows, d = R.ce_fp32(case)
    ref = R.ce_reference(case)
    ratios = (R.ce_dlogits_ratio(case, d), R.loss_ratio(loss, ref["loss"]),
              R.loss_ratio(loss_rows, ref["loss_rows"]))
    print(case, "fp32 evaluation, error / bound (dlogits, loss, loss rows):", ratios)
    assert max(ratios) <= 1.0


def test_ce_per_element_bound_closes_the_max_norm_gap():
    """A gradient with every element below 1e-4 of the maximum zeroed (98 % of them) passes the max-norm check of
    test_kernels_gpu.py test_cross_entropy at its bf16 tolerance and must fail the per-element bound."""
    case = R.CE_CASES[0]
    assert case.dtype == bf and case.V == 50257
    ref = R.ce_reference(case)["dlogits"]
    wrong = torch.where(ref.abs() < 1e-4 * ref.abs().max(), torch.zeros_like(ref), ref)
    live = ref[:, :case.V][ref[:, :case.V].abs().sum(1) > 0]
    assert (live.abs() < 1e-4 * ref.abs().max()).double().mean() > 0.9
    assert R.old_ce_check(wrong, ref) < 1e-2
    assert R.ce_dlogits_ratio(case, wrong) > 100.0
    assert R.ce_dlogits_ratio(case, ref.to(bf)) <= 1.0  # and the rounded reference itself passes


# ------------------------------------------------------------------------------------------------ LayerNorm forward


def test_ln_cases_reach_every_instantiation():
    names = {c.reaches for c in R.LN_FWD_CASES}
    for dt in ("bf16", "f32"):
        assert {f"ln_fwd8_kernel<{dt}, {k}>" for k in (3, 4, 5, 6)} | {f"ln_fwd_kernel<{dt}>"} <= names
    for c in R.LN_FWD_CASES:
        assert c.D % 4 == 0 and c.ldx % 4 == 0 and c.ldy % 4 == 0 and c.ldx >= c.D and c.ldy >= c.D
        assert c.D <= 1024 or c.reaches.startswith("ln_fwd8")
    assert len({c.name for c in R.LN_FWD_CASES}) == len(R.LN_FWD_CASES)
    for D, ldx in R.LN_REJECTED:  # icap_layernorm_fwd's two requirements, restated
        wide = D % 8 == 0 and ldx % 8 == 0
        assert not (D % 4 == 0 and (D <= 1024 or (D <= 1536 and wide)) and ldx % 4 == 0)


@pytest.mark.parametrize("case", [c for c in R.LN_FWD_CASES if c.rows <= 37], ids=repr)
def test_ln_reference_matches_torch(case):
    t = case.inputs()
    ref = R.ln_fwd_reference(case)
    y = torch.nn.functional.layer_norm(t["x"][:case.live].double(), (case.D,), t["gamma"].double(),
                                       t["beta"].double(), R.f32r(R.LN_EPS))
    assert torch.allclose(ref["y"], y, rtol=1e-12, atol=1e-12)
    assert ref["y"].shape == (case.live, case.D) and torch.isfinite(ref["y"]).all()


@pytest.mark.parametrize("case", R.LN_FWD_CASES, ids=repr)
def test_ln_bounds_hold_for_an_fp32_evaluation(case):
    y, mean, rstd = R.ln_fwd_fp32(case)
    ratio, untouched = R.ln_y_check(case, R.ln_layout(case, y))
    rm, rr = R.ln_stats_ratio(case, mean, rstd)
    print(case, "fp32 evaluation, error / bound (y, mean, rstd):", (ratio, rm, rr))
    assert untouched and max(ratio, rm, rr) <= 1.0


def test_ln_check_notices_an_ignored_rowmap():
    """y written in row order, as if y_rowmap were not there: right values, wrong rows."""
    case = next(c for c in R.LN_FWD_CASES if c.rowmap and c.rows_dev is None)
    y, _, _ = R.ln_fwd_fp32(case)
    wrong = torch.full((case.rows, case.ldy), R.SENTINEL, dtype=y.dtype)
    wrong[:, :case.D] = y
    ratio, untouched = R.ln_y_check(case, wrong)
    assert not untouched and ratio > 100.0
    dest = R.ln_dest(case)
    assert int((dest < 0).sum()) == (case.rows + 3) // 4 and sorted(dest[dest >= 0].tolist()) == sorted(
        set(dest[dest >= 0].tolist()))


# ------------------------------------------------------------------------------------------------ AdamW


def test_schedule_closed_form():
    lam = [R.schedule_lam(k, 3, 8) for k in range(10)]
    assert lam == [0.0, 1 / 3, 2 / 3, 1.0, 4 / 5, 3 / 5, 2 / 5, 1 / 5, 0.0, 0.0]
    assert [R.schedule_lam(k, 0, 10) for k in (0, 5, 10, 11)] == [1.0, 0.5, 0.0, 0.0]
    case = R.ADAM_CASES[0]
    ref = R.adamw_reference(case)
    assert [s["lr"] for s in ref] == [R.f32r(case.lr) * l for l in lam[:9]]
    assert ref[0]["lr"] == 0.0 and ref[8]["lr"] == 0.0 and ref[0]["decay"] == 1.0


@pytest.mark.parametrize("case", [c for c in R.ADAM_CASES if c.n <= 4099], ids=repr)
def test_adamw_reference_matches_torch_optim(case):
    p0, grads = case.inputs()
    lr, b1, b2, eps, wd, mx = (R.f32r(v) for v in (case.lr, *case.betas, case.eps, case.weight_decay, case.max_norm))
    pr = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.AdamW([pr], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: R.schedule_lam(s, case.warmup, case.total))
    ref = R.adamw_reference(case)
    for k in range(case.steps):
        pr.grad = grads[k].double().clone()
        norm = torch.nn.utils.clip_grad_norm_([pr], max_norm=mx) if mx > 0 else pr.grad.norm()
        opt.step()
        sched.step()
        st = opt.state[pr]
        assert abs(ref[k]["norm"] - norm.item()) <= 1e-12 * norm.item()
        assert torch.allclose(ref[k]["P"], pr.detach(), rtol=1e-10, atol=1e-14), (case, k)
        assert torch.allclose(ref[k]["M1"], st["exp_avg"], rtol=1e-10, atol=1e-300)
        assert torch.allclose(ref[k]["M2"], st["exp_avg_sq"], rtol=1e-10, atol=1e-300)
        assert ref[k]["step"] == k + 1 == int(st["step"])
    clips = [s["clip"] for s in ref]
    if case.name in ("clip-inactive", "clip-disabled"):
        assert clips == [1.0] * case.steps
    elif case.n == 4099:
        assert max(clips) < 1.0
    assert all((s["decay"] == 1.0) == (wd == 0 or s["lr"] == 0) for s in ref)


@pytest.mark.parametrize("case", R.ADAM_CASES, ids=repr)
def test_adamw_bounds_hold_for_an_fp32_evaluation(case):
    got = R.adamw_fp32(case)
    for k in range(case.steps):
        ratios = R.adam_step_ratios(case, k, got[k])
        print(case, "step", k, "fp32 evaluation, error / bound:", ratios)
        assert max(ratios.values()) <= 1.0, (k, ratios)
    p0, _ = case.inputs()
    if case.warmup:  # lr == 0 at step 0: P is p0 bit for bit while the moments move
        assert torch.equal(got[0]["P"], p0) and got[0]["M1"].abs().max() > 0 and got[0]["M2"].abs().max() > 0


def test_adamw_check_notices_a_missing_warmup():
    """The first-round test's blind spot: a schedule without the warmup branch (lam = (total - k) / (total - warmup)
    from step 0) must fail the state and the update bounds."""
    case = R.ADAM_CASES[0]
    nowarm = R.AdamCase("nowarm", steps=case.steps, warmup=0, total=case.total)
    got = R.adamw_fp32(nowarm)
    r = R.adam_step_ratios(case, 1, got[1])
    assert r["lr"] > 100.0 and r["P"] > 100.0 and r["update"] > 100.0
