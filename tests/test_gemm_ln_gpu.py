"""The LayerNorm forms of icap_gemm on every kernel family per element against the fp64 references of
tests/gemm_ln_refs.py: the statistics producer, the consumer with its row outputs, the decode fold and the fused
LayerNorm of the skinny kernel, and producer launches chained into consumer launches. Each case launches the kernel
instantiation it names (recorded, not assumed); C, aux, the group statistics and the row statistics are checked
element by element against the case's bounds (no max-norm, no exclusions, no retries); and everything a launch must
not touch — padding of C / aux, the NaN guards around and the dead rows of ln_stats_out / ln_mean_out / ln_rstd_out,
every read-only operand — must survive bitwise. One test per family: a handful of small launches."""

import pytest
import torch

import gemm_ln_refs as G
from gemm_helpers import _run
from gemm_ln_refs import CASES, EPS, f32
from icap import ops
from test_gemm_epilogue_gpu import _padded

pytestmark = pytest.mark.gpu

FAMILY_NAMES = sorted({c.family for c in CASES})
GUARD = 4  # fp32 elements (16 bytes: ln_stats_in's alignment) of NaN on either side of a statistics output


def _guarded(shape, dev):
    """(buffer, view): an fp32 output of `shape` inside a NaN-filled buffer with GUARD elements on either side."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=f32, device=dev)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _nan_outside(buf, view, live, what, name):
    """Everything of the buffer but the view's live rows is still NaN; the live rows are finite."""
    per_row = view[0].numel()
    dead = torch.cat([buf[:GUARD], buf[GUARD + live * per_row:]])
    assert torch.isnan(dead).all(), f"{name}: {what} written outside its live rows"
    assert torch.isfinite(view[:live]).all(), f"{name}: {what} not finite (or not written) on a live row"


def _launch(c, dev, x, A=None, stats_in=None):
    """One launch of the case with operands x (A / ln_stats_in: device tensors of a chain's first launch). Returns
    (outputs on the CPU, C view on the device, statistics view on the device)."""
    M, N, K, lay = c.M, c.N, c.K, c.layout
    ldc, ldaux, ldr, _ = c.lds()
    A = x.A.to(dev) if A is None else A
    B, bias = x.B.to(dev), x.bias.to(dev)
    Cbuf, C = _padded((M, N, c.c_dt), ldc, lay.off, dev)
    rbuf, resid = _padded(x.resid, ldr, lay.off, dev)
    kw = dict(c.kw, alpha=c.alpha, M=M, N=N, K=K, bias=bias, resid=resid, act=c.act)
    padded, nans, ro = [(Cbuf, "C")], [], [(A, "A"), (B, "B"), (bias, "bias"), (rbuf, "resid")]
    aux = stats = None
    if c.aux:
        auxbuf, aux = _padded((M, N, c.c_dt), ldaux, lay.off, dev)
        kw["aux"] = aux
        padded.append((auxbuf, "aux"))
    if c.form == "producer":
        sbuf, stats = _guarded((M, N // 32, 2), dev)
        kw["ln_stats_out"] = stats
        nans.append((sbuf, stats, "ln_stats_out"))
    elif c.form == "fused":
        gamma, beta = x.gamma.to(dev), x.beta.to(dev)
        kw["ln"] = (gamma, beta, EPS)
        ro += [(gamma, "ln_gamma"), (beta, "ln_beta")]
    else:
        wsum = x.wsum.to(dev)
        kw["ln_fold"] = (wsum, EPS)
        ro.append((wsum, "ln_wsum"))
    if c.rows_out:
        stats_in = x.stats_given.to(dev) if stats_in is None else stats_in
        assert stats_in.data_ptr() % 16 == 0 and stats_in.is_contiguous()
        mbuf, mean = _guarded((M,), dev)
        rsbuf, rstd = _guarded((M,), dev)
        kw.update(ln_stats_in=stats_in, ln_rows_out=(mean, rstd))
        ro.append((stats_in, "ln_stats_in"))
        nans += [(mbuf, mean, "ln_mean_out"), (rsbuf, rstd, "ln_rstd_out")]
    if c.m_dev:
        kw["m_dev"] = torch.tensor([c.live], dtype=torch.int32, device=dev)
        kw["m_hint"] = c.live
    before = [b.clone() for b, _ in padded + ro]
    names = _run(lambda: ops.gemm(A, B, C, **kw))
    torch.cuda.synchronize()
    if c.form == "producer" and c.kind is None:  # a chain's first launch: some producer kind of the planner's choice
        assert len(names) == 1 and G._kind_of(names[0]) == G.LNS, (c.name, names)
    else:
        assert names == [c.kernel()], (c.name, names, c.kernel())
    for (buf, what), b0 in zip(padded + ro, before):
        if what in ("C", "aux"):
            keep = torch.ones(buf.shape, dtype=torch.bool, device=dev)
            keep[:c.live, lay.off:lay.off + N] = False
            assert torch.equal(buf[keep], b0[keep]), f"{c.name}: {what} written outside its live elements"
        else:
            assert torch.equal(buf, b0), f"{c.name}: {what} modified"
    for buf, view, what in nans:
        _nan_outside(buf, view, c.live, what, c.name)
    got = {"C": C.cpu()}
    if aux is not None:
        got["aux"] = aux.cpu()
    if stats is not None:
        got["stats"] = stats.cpu()
    if c.rows_out:
        got["mean"], got["rstd"] = mean.cpu(), rstd.cpu()
    return got, C, stats


def _run_case(c, dev):
    if c.form != "chain":
        got, _, _ = _launch(c, dev, c.inputs())
        return G.check(c, got)
    p = c.producer()
    p.kind = None
    first, C1, st1 = _launch(p, dev, p.inputs())
    w1 = G.check(p, first)
    assert max(w1.values()) <= 1.0, (c.name, "producer", w1)
    x = G.chain_inputs(c, first["C"], first["stats"])
    got, _, _ = _launch(c, dev, x, A=C1, stats_in=st1)
    return G.check(c, got, x)


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_ln_forms_per_element(dev, family):
    worst = {}
    for c in CASES:
        if c.family == family:
            try:
                worst[c] = _run_case(c, dev)
            except AssertionError:
                raise
            except Exception as e:  # a launch or device error: nothing more runs on this device
                pytest.exit(f"{c.name}: {type(e).__name__}: {e}", returncode=3)
            print(f"{c.name}: worst ratios " + " ".join(f"{k} {v:.3f}" for k, v in worst[c].items()))
    by = {}
    for c, w in worst.items():
        for k, v in w.items():
            key = (c.form if family != "skinny" else f"{c.form} {G.R.dt_name(c.in_dt)}/{G.R.dt_name(c.c_dt)}", k)
            by[key] = max(by.get(key, 0.0), v)
    print(f"family {family}, {len(worst)} cases: " + "; ".join(f"{f} {k} {v:.3f}" for (f, k), v in sorted(by.items())))
    bad = {c.name: w for c, w in worst.items() if not max(w.values()) <= 1.0}
    assert not bad, bad
