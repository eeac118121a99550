"""The kernels between the last GPT-2 block and the parameter update — icap_layernorm_fwd, icap_cross_entropy,
icap_adamw_step — against the fp64 references, cases and bounds of tests/loss_refs.py (its docstring derives the
bounds; test_loss_refs_cpu.py checks references and bounds without a GPU). Every test prints its worst ratio of
error to bound before it asserts.

Worst error / bound measured on an MI355X when the file was added (all bounds as loss_refs.py derives them; the
bf16 figures sit just under 1 because half an ulp of the one rounding is most of a bf16 bound):
  cross entropy  dlogits: ce_bf16_reg_kernel<13> 0.990, ce_kernel<bf16> 0.991, ce_kernel<float> 0.159;
                 per-row losses 0.048, scalar loss 0 (equal to the fp32-rounded reference in every case);
                 in place == out of place bit for bit in every case
  LayerNorm fwd  y: bf16 0.989 (8-wide) / 0.988 (4-wide), fp32 0.0155 / 0.0187; mean 0.0275; rstd 0.0208
  AdamW          P 0.194, exp_avg 0.411 (n = 1), exp_avg_sq 0.266, update 0.036, tail elements 0.072,
                 norm 0.055, clip 0.080, lr / step_size / bc2_sqrt / decay 0.195"""

import pytest
import torch

import loss_refs as R
from icap import _lib as L
from icap import ops

pytestmark = pytest.mark.gpu

bf, f32 = torch.bfloat16, torch.float32


def bits(t):
    return t.view(torch.int16 if t.dtype == bf else torch.int32)


# ------------------------------------------------------------------------------------------------ cross entropy


def ce_buffer(case, dev, values, offset):
    """A [rows, ld] view at element `offset` of a fresh 16-byte aligned flat buffer holding `values`."""
    flat = torch.zeros(case.rows * case.ld + 8, dtype=case.dtype, device=dev)
    assert flat.data_ptr() % 16 == 0
    v = flat[offset:offset + case.rows * case.ld].view(case.rows, case.ld)
    v.copy_(values)
    return v


def ce_run(case, dev, inplace):
    """One call. Returns (loss [1], per-row losses [rows], dlogits [rows, ld] or None, logits after the call)."""
    t = case.inputs()
    x0 = t["logits"].to(dev)
    labels = t["labels"].to(dev)
    nv = torch.tensor([R.ce_reference(case)["n_valid"]], dtype=torch.int32, device=dev)
    rows_dev = None if case.rows_dev is None else torch.tensor([case.rows_dev], dtype=torch.int32, device=dev)
    loss = torch.full((1,), R.STAT_SENTINEL, device=dev)
    assert ops.cross_entropy_workspace(case.rows) == 4 * case.rows
    ws = torch.full((case.rows,), R.STAT_SENTINEL, dtype=f32, device=dev)
    logits = ce_buffer(case, dev, x0, case.offset if inplace else 0)
    if not case.dlogits:
        dl = None
    elif inplace:
        dl = logits
    else:
        dl = ce_buffer(case, dev, torch.full_like(x0, R.SENTINEL), case.offset)
    ops.cross_entropy(logits, case.V, labels, nv, loss, dl, ws, grad_scale=case.grad_scale, rows_dev=rows_dev)
    torch.cuda.synchronize()
    return loss, ws, dl, logits


@pytest.mark.parametrize("case", R.CE_CASES, ids=repr)
def test_cross_entropy(dev, case):
    ref = R.ce_reference(case)
    n, V = case.live, case.V
    t = case.inputs()
    loss, rows, dl, logits = ce_run(case, dev, inplace=False)
    r_loss, r_rows = R.loss_ratio(loss, ref["loss"]), R.loss_ratio(rows[:n], ref["loss_rows"])
    print(f"{case} -> {case.reaches}: loss {loss.item():.9g} (ref {ref['loss']:.9g}), error / bound: "
          f"loss {r_loss:.3g}, loss rows {r_rows:.3g}")
    assert torch.equal(bits(logits.cpu()), bits(t["logits"]))  # the input is only read
    assert torch.equal(rows[n:].cpu(), torch.full((case.rows - n,), R.STAT_SENTINEL))
    assert r_loss <= 1.0 and r_rows <= 1.0
    if not case.dlogits:
        return
    got = dl.cpu()
    r_d = R.ce_dlogits_ratio(case, got[:n])
    print(f"{case}: dlogits error / bound {r_d:.3g}")
    ignored = t["labels"][:n] < 0
    assert torch.equal(got[:n][ignored], torch.zeros_like(got[:n][ignored]))
    assert torch.equal(got[:n, V:], torch.zeros_like(got[:n, V:]))
    assert torch.equal(got[n:], torch.full_like(got[n:], R.SENTINEL))
    assert r_d <= 1.0
    # dlogits = logits, as GPT2.forward_train calls it: the same bits
    loss2, rows2, dl2, _ = ce_run(case, dev, inplace=True)
    assert torch.equal(loss2, loss) and torch.equal(rows2, rows)
    assert torch.equal(bits(dl2[:n].cpu()), bits(got[:n]))
    assert torch.equal(bits(dl2[n:].cpu()), bits(t["logits"][n:]))  # NaN rows past rows_dev: untouched


# ------------------------------------------------------------------------------------------------ LayerNorm forward


def strided(values, ld, dev, fill):
    """values [rows, D] inside a [rows, ld] buffer filled with `fill` (16-byte aligned base)."""
    rows, D = values.shape
    buf = torch.full((rows, ld), fill, dtype=values.dtype, device=dev)
    assert buf.data_ptr() % 16 == 0
    buf[:, :D] = values.to(dev)
    return buf


@pytest.mark.parametrize("case", R.LN_FWD_CASES, ids=repr)
def test_layernorm_fwd(dev, case):
    t = case.inputs()
    rows, D = case.rows, case.D
    xb = strided(t["x"], case.ldx, dev, 3.0)
    yb = torch.full((rows, case.ldy), R.SENTINEL, dtype=case.dtype, device=dev)
    mean = torch.full((rows,), R.STAT_SENTINEL, device=dev) if case.stats else None
    rstd = torch.full((rows,), R.STAT_SENTINEL, device=dev) if case.stats else None
    rowmap = None if t["rowmap"] is None else t["rowmap"].to(dev)
    rows_dev = None if case.rows_dev is None else torch.tensor([case.rows_dev], dtype=torch.int32, device=dev)
    ops.layernorm_fwd(xb[:, :D], t["gamma"].to(dev), t["beta"].to(dev), R.LN_EPS, yb[:, :D], mean, rstd, rows=rows,
                      y_rowmap=rowmap, rows_dev=rows_dev)
    torch.cuda.synchronize()
    ratio, untouched = R.ln_y_check(case, yb.cpu())
    rm = rr = 0.0
    if case.stats:
        rm, rr = R.ln_stats_ratio(case, mean, rstd)
        assert torch.equal(mean[case.live:].cpu(), torch.full((rows - case.live,), R.STAT_SENTINEL))
        assert torch.equal(rstd[case.live:].cpu(), torch.full((rows - case.live,), R.STAT_SENTINEL))
    print(f"{case} -> {case.reaches}: error / bound y {ratio:.3g}, mean {rm:.3g}, rstd {rr:.3g}")
    assert untouched, "an element outside the stored rows / columns changed"
    assert ratio <= 1.0 and rm <= 1.0 and rr <= 1.0


@pytest.mark.parametrize("dtype", [bf, f32], ids=R.dt_name)
@pytest.mark.parametrize("D,ldx", R.LN_REJECTED)
def test_layernorm_fwd_rejects(dev, dtype, D, ldx):
    x = torch.ones((9, ldx), dtype=dtype, device=dev)
    y = torch.full((9, ldx), R.SENTINEL, dtype=dtype, device=dev)
    g = torch.ones(D, device=dev)
    with pytest.raises(L.IcapError):
        ops.layernorm_fwd(x[:, :D], g, g, R.LN_EPS, y[:, :D], None, None)
    torch.cuda.synchronize()
    assert torch.equal(y, torch.full_like(y, R.SENTINEL))


# ------------------------------------------------------------------------------------------------ AdamW


@pytest.mark.parametrize("case", R.ADAM_CASES, ids=repr)
def test_adamw(dev, case):
    p0, grads = case.inputs()
    n = case.n
    P, M1, M2 = p0.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    st = torch.zeros(16, dtype=f32, device=dev)
    ws = torch.empty(ops.adamw_workspace(n), dtype=torch.uint8, device=dev)
    out16 = torch.full((n,), R.SENTINEL, dtype=bf, device=dev) if case.bf16_out else None
    worst = {}
    for k in range(case.steps):
        g = grads[k].to(dev)
        ops.adamw_step(P, g, M1, M2, st, ws, bf16_out=out16, **case.kwargs())
        torch.cuda.synchronize()
        assert torch.equal(g.cpu(), grads[k])  # the gradient is only read
        s = st.cpu()
        got = dict(P=P, M1=M1, M2=M2, step=s[:2].view(torch.int64).item(),
                   **{f: s[2 + i].item() for i, f in enumerate(R.ADAM_FIELDS)})
        ratios = R.adam_step_ratios(case, k, got)
        print(f"{case} step {k}: error / bound", {f: float(f"{v:.3g}") for f, v in ratios.items()})
        for f, v in ratios.items():
            worst[f] = max(worst.get(f, 0.0), v)
        assert max(ratios.values()) <= 1.0, (k, ratios)
        if out16 is not None:
            assert torch.equal(out16, P.to(bf))
        if k == 0 and case.warmup:  # lr == 0: P unchanged bit for bit, the moments move
            assert torch.equal(P.cpu(), p0) and M1.abs().max() > 0 and M2.abs().max() > 0
        assert torch.equal(s[8:], torch.zeros(8))  # the padding of the 64-byte state stays zero
    print(f"{case}: worst error / bound", {f: float(f"{v:.3g}") for f, v in worst.items()})
