"""icap_caption_score and icap_caption_target_ranges alone, on designed logits (tests/score_refs.py) against the fp64
restatement. Shapes: V = 50257 / ld = 50304 (the V % 8 = 1 tail and padding columns holding 1e30 / NaN), V = 512,
V = 13 / ld = 16; bf16 (the register-resident row kernel for all three) and fp32 (the streaming one). Layouts: the
padded grid with -100 rows between the targets, and the compact rows with rows_dev < rows (rows past it NaN, output
elements past it keep the sentinel). Bounds: score_refs' docstring."""

import functools

import numpy as np
import pytest
import torch

import loss_refs
import score_refs as R
from icap import ops

pytestmark = pytest.mark.gpu
bf, f32 = torch.bfloat16, torch.float32
SHAPES = [(50257, 50304), (512, 512), (13, 16)]
B, P, Lc, S = 5, 2, 10, 12
SENT = loss_refs.STAT_SENTINEL


@functools.lru_cache(maxsize=None)
def case(V, ld, dtype, nonfinite=True):
    """Host inputs and fp64 references of one shape, shared by the tests (never modified)."""
    xt, yt = R.designed_targets(V, ld, dtype, nonfinite=nonfinite)
    xp, yp, rp = R.padded_layout(xt, yt, S)
    xc, yc, rc, live = R.compact_layout(xt, yt)
    slot = torch.full((B * S,), -1, dtype=torch.int32)
    slot[yp >= 0] = torch.arange(live, dtype=torch.int32)
    nll_t, hit_t = R.row_scores(xt, yt, V)
    nll_p = torch.zeros(B * S, dtype=torch.float64)
    nll_p[yp >= 0] = nll_t
    hit_p = torch.zeros(B * S, dtype=torch.bool)
    hit_p[yp >= 0] = hit_t
    tgt = (yp >= 0).view(B, S)
    tlp = torch.where(tgt[:, P - 1: P - 1 + Lc], -nll_p.view(B, S)[:, P - 1: P - 1 + Lc],
                      torch.zeros((B, Lc), dtype=torch.float64))
    seq = R.seq_sum(nll_p.view(B, S))
    return dict(V=V, ld=ld, dtype=dtype, xp=xp, yp=yp, rp=rp, xc=xc, yc=yc, rc=rc, live=live, slot=slot,
                nll_t=nll_t, hit_t=hit_t, nll_p=nll_p, hit_p=hit_p, tlp=tlp, seq=seq,
                ntok=tgt.sum(1), ncor=hit_p.view(B, S).sum(1))


def run(dev, c, layout, totals=None):
    """One call; returns host copies of every output (the workspace as (row nll fp32, row hit int32))."""
    compact = layout == "compact"
    x = (c["xc"] if compact else c["xp"]).to(dev)
    y = (c["yc"] if compact else c["yp"]).to(dev)
    ranges = (c["rc"] if compact else c["rp"]).to(dev)
    rows = x.shape[0]
    nll = torch.full((B,), SENT, dtype=f32, device=dev)
    ntok = torch.full((B,), -7, dtype=torch.int32, device=dev)
    ncor = torch.full((B,), -7, dtype=torch.int32, device=dev)
    tlp = torch.full((B, Lc), SENT, dtype=f32, device=dev)
    ws = torch.full((ops.caption_score_workspace(rows) // 4,), SENT, dtype=f32, device=dev)
    rows_dev = torch.tensor([c["live"]], dtype=torch.int32, device=dev) if compact else None
    slot = c["slot"].to(dev) if compact else None
    ops.caption_score(x, c["V"], y, ranges, nll, ntok, ncor, ws, rows_dev=rows_dev, token_logprobs=tlp, P=P, Lc=Lc,
                      row_slot=slot, totals=totals)
    torch.cuda.synchronize(dev)
    w = ws.cpu()
    return dict(nll=nll.cpu(), ntok=ntok.cpu(), ncor=ncor.cpu(), tlp=tlp.cpu(), row_nll=w[:rows],
                row_hit=w[rows:].view(torch.int32), rows=rows)


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("layout", ["padded", "compact"])
@pytest.mark.parametrize("dtype", [bf, f32], ids=["bf16", "f32"])
@pytest.mark.parametrize("V,ld", SHAPES)
def test_score_against_fp64(dev, V, ld, dtype, layout):
    c = case(V, ld, dtype)
    o = run(dev, c, layout)
    live = c["live"]
    if layout == "compact":
        ref_rows, ref_hit, n = c["nll_t"], c["hit_t"], live
        ranges = list(zip(c["rc"][:-1].tolist(), c["rc"][1:].tolist()))
        # rows at or beyond rows_dev: neither read (they hold NaN and label 0) nor written
        assert bool((o["row_nll"][n:] == SENT).all())
        assert torch.equal(bits(o["row_hit"][n:]), bits(torch.full((o["rows"] - n,), SENT)))
    else:
        ref_rows, ref_hit, n = c["nll_p"], c["hit_p"], B * S
        ranges = [(b * S, (b + 1) * S) for b in range(B)]
        assert bool((o["row_nll"][c["yp"] < 0] == 0).all())      # ignored rows score 0
    got_rows = o["row_nll"][:n]
    assert R.same_nonfinite(got_rows, ref_rows)
    row_ratio = loss_refs.loss_ratio(*R.finite(got_rows, ref_rows))
    seq_ratio = R.seq_ratio(o["nll"], ref_rows, ranges)
    print(f"V={V} {loss_refs.dt_name(dtype)} {layout}: row ratio {row_ratio:.3f} seq ratio {seq_ratio:.3f}")
    assert row_ratio <= 1.0
    assert R.same_nonfinite(o["nll"], c["seq"]) and seq_ratio <= 1.0
    assert float(o["nll"][0]) == 0.0                              # the sequence without a target
    assert torch.equal(o["row_hit"][:n].bool(), ref_hit)
    assert torch.equal(o["ntok"].long(), c["ntok"]) and torch.equal(o["ncor"].long(), c["ncor"])
    assert o["ntok"].tolist() == list(R.SEQ_TARGETS)
    # token_logprobs: the zero pattern exactly, the values within the per-row bound
    assert torch.equal(o["tlp"] == 0, c["tlp"] == 0)
    assert R.same_nonfinite(o["tlp"], c["tlp"])
    assert loss_refs.loss_ratio(*R.finite(o["tlp"], c["tlp"])) <= 1.0
    # the per-sequence value is the double sum of the stored fp32 rows in row order, rounded once
    for b, (r0, r1) in enumerate(ranges):
        acc = 0.0
        for r in range(r0, r1):
            if (c["yc"] if layout == "compact" else c["yp"])[r] >= 0:
                acc += float(o["row_nll"][r])
        want = torch.tensor(acc, dtype=torch.float64).float()
        assert torch.equal(bits(o["nll"][b: b + 1]), bits(want.reshape(1))), b


@pytest.mark.parametrize("dtype", [bf, f32], ids=["bf16", "f32"])
def test_padded_and_compact_forms_agree_bitwise(dev, dtype):
    c = case(50257, 50304, dtype)
    a, b = run(dev, c, "padded"), run(dev, c, "compact")
    for k in ("nll", "ntok", "ncor", "tlp"):
        assert torch.equal(bits(a[k]), bits(b[k])), k


@pytest.mark.parametrize("layout", ["padded", "compact"])
@pytest.mark.parametrize("dtype", [bf, f32], ids=["bf16", "f32"])
def test_totals_and_reproducibility(dev, dtype, layout):
    """totals after two calls is the double sum, in sequence order, of both calls' fp32 nll (and counts), bitwise;
    two runs give the same bits. Finite rows only, so the sum says something; with the non-finite rows it is NaN."""
    c = case(512, 512, dtype, nonfinite=False)
    totals = torch.zeros(3, dtype=torch.float64, device=dev)
    o1 = run(dev, c, layout, totals)
    o2 = run(dev, c, layout, totals)
    for k in ("nll", "ntok", "ncor", "tlp", "row_nll", "row_hit"):
        assert torch.equal(bits(o1[k]), bits(o2[k])), k
    a = [0.0, 0.0, 0.0]
    for o in (o1, o2):
        for b in range(B):
            a[0] += float(o["nll"][b])
            a[1] += float(o["ntok"][b])
            a[2] += float(o["ncor"][b])
    got = totals.cpu()
    assert torch.equal(got.view(torch.int64), torch.tensor(a, dtype=torch.float64).view(torch.int64)), (got, a)
    assert got[1] == 30 and np.isfinite(a[0])
    t2 = torch.zeros(3, dtype=torch.float64, device=dev)
    run(dev, case(512, 512, dtype), layout, t2)
    t2 = t2.cpu()
    assert torch.isnan(t2[0]) and t2[1] == 15 and t2[2] == float(case(512, 512, dtype)["ncor"].sum())


def test_first_bf16_shape_past_the_register_form(dev):
    """V = 8 * 512 * 13 + 8 takes the streaming kernel for bf16 (the register form holds 13 groups per thread)."""
    V = 8 * 512 * 13 + 8
    xt, yt = R.designed_targets(V, V, bf)
    nll, hit = R.row_scores(xt, yt, V)
    n = xt.shape[0]
    ranges = torch.tensor([0, n], dtype=torch.int32, device=dev)
    out = torch.zeros(1, dtype=f32, device=dev)
    ntok, ncor = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.zeros(ops.caption_score_workspace(n) // 4, dtype=f32, device=dev)
    ops.caption_score(xt.to(dev), V, yt.to(dev), ranges, out, ntok, ncor, ws)
    rows = ws.cpu()[:n]
    assert R.same_nonfinite(rows, nll) and loss_refs.loss_ratio(*R.finite(rows, nll)) <= 1.0
    assert torch.equal(ws.cpu()[n:].view(torch.int32).bool(), hit)
    assert int(ntok) == n and int(ncor) == int(hit.sum())


def _ranges_case(nB, S_, seed, packed):
    """Random target patterns (some sequences empty): row_slot over the grid rows, expected ranges."""
    g = torch.Generator().manual_seed(seed)
    tgt = torch.rand((nB, S_), generator=g) < 0.4
    tgt[::5] = False
    tgt[:, 0] = False
    if not packed:
        flat = tgt.reshape(-1)
        slot = torch.where(flat, torch.cumsum(flat.int(), 0) - 1, torch.full_like(flat.int(), -1)).int()
        off = ln = None
    else:
        pos = torch.arange(1, S_ + 1)
        ln = torch.clamp((tgt.int() * pos).max(1).values, min=3).int()   # live prefix, at least 3 rows
        off = (torch.cumsum(ln, 0) - ln).int()
        flat = torch.cat([tgt[b, : int(ln[b])] for b in range(nB)])
        slot = torch.full((nB * S_,), -1, dtype=torch.int32)
        slot[: flat.numel()] = torch.where(flat, torch.cumsum(flat.int(), 0) - 1, torch.full_like(flat.int(), -1))
    want = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(tgt.sum(1), 0)]).int()
    return slot, off, ln, want


@pytest.mark.parametrize("nB,S_", [(1, 7), (5, 12), (64, 17), (130, 62), (300, 9), (3, 150)])
def test_target_ranges(dev, nB, S_):
    """The three forms against a host cumulative sum; B past 64 and past 16 x 64 crosses the scan's chunks, S past
    64 the count's."""
    out = torch.full((nB + 2,), -7, dtype=torch.int32, device=dev)
    ops.caption_target_ranges(nB, S_, out)
    assert out.cpu().tolist() == [b * S_ for b in range(nB + 1)] + [-7]
    for packed in (False, True):
        slot, off, ln, want = _ranges_case(nB, S_, 11 + nB, packed)
        out.fill_(-7)
        seqs = (off.to(dev), ln.to(dev)) if packed else None
        ops.caption_target_ranges(nB, S_, out, row_slot=slot.to(dev), seqs=seqs)
        assert out.cpu().tolist() == want.tolist() + [-7], packed
