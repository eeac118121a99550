"""Training-time attention, forward and backward, per element against fp64 on every dispatch path
(csrc/attention_mfma.hip fwd v1 / v2 / v3, bwd v1 / v2, the packed short / long passes; csrc/attention.hip's VALU
forward with and without query tiling and VALU backward).

Bound, weights, cases and the kernel each case reaches: tests/attn_refs.py (checked on the CPU by
test_attn_refs_cpu.py, which also shows the old whole-tensor rel_err limits accepting a dropped key and zeroed dK
rows). Here every element of out, lse, dQ, dK and dV must satisfy |got - ref| <= a |ref| + b A, exact zeros where
the bound is zero, -inf in lse exactly where no key is allowed. Outputs live in buffers filled with a sentinel
(777, exact in bf16) with pad columns and a spare row; everything a kernel has no business writing must still hold
it. Unused input rows are NaN: data a kernel must not read, never an address.

Every pointer and stride here is one the dispatch accepts and the chosen kernel's vector accesses are aligned for.
"""

import pytest
import torch

import attn_refs as A
from icap import _lib as L
from icap import ops

pytestmark = pytest.mark.gpu

SENT = 777.0
NAN = float("nan")


def _bufs(case, dev, nrows):
    """Sentinel-filled out [nrows + 1, D + PAD], dqkv [nrows + 1, 3D + PAD], lse [B*H*S + 16] and the views a launch
    gets. off2 (first-generation forward): out starts 2 elements (4 bytes) into each row."""
    D = case.H * case.hd
    obuf = torch.full((nrows + 1, D + A.PAD), SENT, dtype=case.dtype, device=dev)
    gbuf = torch.full((nrows + 1, 3 * D + A.PAD), SENT, dtype=case.dtype, device=dev)
    lbuf = torch.full((case.B * case.H * case.S + 16,), SENT, device=dev)
    c0 = 2 if case.off2 else 0
    out = obuf[:nrows, c0:c0 + D]
    assert out.data_ptr() % 16 == (4 if case.off2 else 0) and obuf.stride(0) % 8 == 0 and gbuf.stride(0) % 8 == 0
    return obuf, gbuf, lbuf, out, gbuf[:nrows, :3 * D], lbuf[: case.B * case.H * case.S], c0


def _untouched(obuf, gbuf, lbuf, case, nrows, c0, written_rows=None, bwd=True):
    D = case.H * case.hd
    assert (obuf[:, :c0] == SENT).all() and (obuf[:, c0 + D:] == SENT).all() and (obuf[nrows:] == SENT).all()
    assert (lbuf[case.B * case.H * case.S:] == SENT).all()
    assert (gbuf[:, 3 * D:] == SENT).all() and (gbuf[nrows:] == SENT).all()
    if not bwd:
        assert (gbuf == SENT).all()
    if written_rows is not None:  # packed: rows that belong to no sequence
        assert (obuf[written_rows:] == SENT).all() and (gbuf[written_rows:] == SENT).all()


def _dev_drop(case, dev):
    """ops.Dropout of a dropout_refs.AttnCase: its descriptor, with the device counter where it has one."""
    d, ctr = case.desc()
    t = None if ctr is None else torch.full((1,), ctr, dtype=torch.int64, device=dev)
    return ops.Dropout(d.p, d.seed, d.offset, t)


def _check(label, kernel, r):
    """Prints one line per launch — case, kernel reached, error / bound ratio per output — and asserts the bound."""
    print(f"{label} [{kernel}]: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), (label, kernel, r)


def _run(dev, case):
    """forward + each backward form of a padded case; asserts the bound per element and the sentinels."""
    B, S, H, hd = case.B, case.S, case.H, case.hd
    D, n = H * hd, B * S
    qkv_c, dout_c = case.inputs()
    qkv = torch.full((n + 1, 3 * D), NAN, dtype=case.dtype, device=dev)
    qkv[:n] = qkv_c.to(dev)
    qkv, dout = qkv[:n], dout_c.to(dev)
    assert qkv.data_ptr() % 16 == 0 and dout.data_ptr() % 16 == 0
    km = case.key_mask()
    drop = ops.NO_DROP if case.keep is None else _dev_drop(case.c, dev)
    kw = dict(B=B, S=S, H=H, hd=hd, scale=case.scale, causal=case.causal, key_mask=None if km is None else km.to(dev),
              drop=drop)
    ref = A.reference(case)
    expect = getattr(case, "expect", {})
    obuf, gbuf, lbuf, out, dqkv, lse, c0 = _bufs(case, dev, n)
    ops.attention_fwd(qkv, out, lse=lse, **kw)
    torch.cuda.synchronize()
    _untouched(obuf, gbuf, lbuf, case, n, c0, bwd=False)
    _check(f"{case} fwd", expect.get("fwd", case.family), A.ratios(case.family, dict(out=out, lse=lse), ref))
    for form in case.forms:
        gbuf.fill_(SENT)
        ops.attention_bwd(qkv, dout, lse, dqkv, out=out if form == "O" else None, **kw)
        torch.cuda.synchronize()
        _untouched(obuf, gbuf, lbuf, case, n, c0)
        got = dict(dq=dqkv[:, :D], dk=dqkv[:, D:2 * D], dv=dqkv[:, 2 * D:])
        _check(f"{case} bwd {form}", expect.get(form, f"{case.family} {form}"),
               A.ratios(case.family, got, ref, form=form))


@pytest.mark.parametrize("case", A.CASES, ids=repr)
def test_attention_per_element(dev, case):
    _run(dev, case)


@pytest.mark.parametrize("case", A.DROP_CASES, ids=repr)
def test_attention_dropout_per_element(dev, case):
    """dropout_refs' cases (the device's own mask, p = 0.1 / 0.5) under the per-element bound, weights built from
    the dropped probabilities."""
    _run(dev, case)


@pytest.mark.parametrize("case", A.PACKED_CASES, ids=repr)
def test_attention_packed_per_element(dev, case):
    """A packed launch against fp64 directly (not against the padded launch): live rows per element, rows that
    belong to no sequence untouched, lse at the positions a packed launch writes (q < seq_len[b])."""
    B, S, H, hd = case.B, case.S, case.H, case.hd
    D, n, nr = H * hd, case.n, B * S
    qkv_p, dout_p = case.inputs()
    live = case.live_rows()
    qkv = torch.full((nr, 3 * D), NAN, dtype=case.dtype, device=dev)
    dout = torch.full((nr, D), NAN, dtype=case.dtype, device=dev)
    qkv[:n], dout[:n] = qkv_p[live].to(dev), dout_p[live].to(dev)
    assert qkv.data_ptr() % 16 == 0 and dout.data_ptr() % 16 == 0
    kmp = torch.zeros(nr, dtype=torch.int32)
    kmp[:n] = case.key_mask().reshape(-1)[live]
    i32 = dict(dtype=torch.int32, device=dev)
    seqs = (torch.tensor(case.off, **i32), torch.tensor(case.lens, **i32))
    kw = dict(B=B, S=S, H=H, hd=hd, scale=case.scale, causal=case.causal, key_mask=kmp.to(dev), seqs=seqs,
              short_only=case.short_only)
    ref = A.reference(case)
    obuf, gbuf, lbuf, out, dqkv, lse, c0 = _bufs(case, dev, nr)
    ops.attention_fwd(qkv, out, lse=lse, **kw)
    torch.cuda.synchronize()
    _untouched(obuf, gbuf, lbuf, case, nr, c0, written_rows=n, bwd=False)
    ops.attention_bwd(qkv, dout, lse, dqkv, out=out, **kw)
    torch.cuda.synchronize()
    _untouched(obuf, gbuf, lbuf, case, nr, c0, written_rows=n)
    got = dict(out=out, lse=lse, dq=dqkv[:, :D], dk=dqkv[:, D:2 * D], dv=dqkv[:, 2 * D:])
    passes = "+".join(A.packed_passes(S, case.short_only)) if case.family == "mfma" else "valu"
    _check(f"{case} fwd+bwd O", f"packed {case.family} {passes}",
           A.ratios(case.family, got, ref, sel=(torch.arange(n), live), lse_sel=(case.live_lse(), case.live_lse())))


def test_fp32_backward_refused_past_lds(dev):
    """fp32 backward at S = 93, hd 64: 4 S (hd + 1) + 2 S^2 floats pass the 160 KB of LDS (S = 92 is the last that
    fits and runs above). The check is on the host, before any launch: an IcapError, dqkv untouched."""
    B, S, H, hd = 2, 93, 3, 64
    D = H * hd
    assert A.valu_bwd_lds(92, hd) <= A.LDS_CAP < A.valu_bwd_lds(S, hd)
    qkv = torch.zeros((B * S, 3 * D), device=dev)
    dout = torch.zeros((B * S, D), device=dev)
    lse = torch.zeros(B * H * S, device=dev)
    dqkv = torch.full_like(qkv, SENT)
    with pytest.raises(L.IcapError):
        ops.attention_bwd(qkv, dout, lse, dqkv, B=B, S=S, H=H, hd=hd, scale=hd ** -0.5, causal=True)
    torch.cuda.synchronize()
    assert (dqkv == SENT).all()
