"""Every dropout-bearing kernel against an fp64 reference that uses the device's own mask (tests/dropout_refs.py:
the restated counter-based hash, checked on the CPU by test_dropout_refs_cpu.py).

A forward / backward mask mismatch (a transposed q*S+k, ld in place of N, a packed row in place of a padded one, the
device counter read in one direction only) would still train, and statistics or path-equality tests pass on it; here
it moves the result by more than 10x each bound (shown on the CPU). Each family runs once with a seed that has bits
above 32 set at offset 5 + 2^40 and once with a device counter holding 3; p = 0.1, and 0.5 for one case per family.
Bounds are those of the same kernels' dropout-free tests in test_kernels_gpu.py (dropout_refs.*_tols). Which
kernel a shape reaches is listed beside the cases in dropout_refs.py (the dispatch rules of
csrc/attention_mfma.hip mfma_attention_launch, csrc/attention.hip, csrc/layernorm.hip icap_layernorm_bwd).
"""

import numpy as np
import pytest
import torch

import dropout_refs as R
from icap import _lib as L
from icap import ops

pytestmark = pytest.mark.gpu


def dev_drop(case_or_desc, dev):
    d, ctr = case_or_desc.desc() if hasattr(case_or_desc, "desc") else case_or_desc
    t = None if ctr is None else torch.full((1,), ctr, dtype=torch.int64, device=dev)
    return ops.Dropout(d.p, d.seed, d.offset, t)


def lse_err(lse, ref):
    """max |d| over the finite entries; the -inf entries (no allowed key) must coincide."""
    lse, ref = lse.detach().double().cpu(), ref.double()
    inf = ref == float("-inf")
    assert torch.equal(lse == float("-inf"), inf)
    assert not torch.isnan(lse).any()
    return (lse[~inf] - ref[~inf]).abs().max().item()


def run_case(dev, case):
    """forward + (both) backwards of an AttnCase on the device: (out, lse, {form: dqkv})."""
    qkv, dout = (x.to(dev) for x in case.inputs())
    km = case.key_mask()
    km = None if km is None else km.to(dev)
    B, S, H, hd = case.B, case.S, case.H, case.hd
    kw = dict(B=B, S=S, H=H, hd=hd, scale=case.scale, causal=case.causal, key_mask=km, drop=dev_drop(case, dev))
    out = torch.full((B * S, H * hd), float("nan"), device=dev, dtype=case.dtype)
    lse = torch.full((B * H * S,), float("nan"), device=dev)
    ops.attention_fwd(qkv, out, lse=lse, **kw)
    grads = {}
    if case.bwd:
        # without O: bwd_kernel<64 / 96> (bf16; the VALU kernel at hd 128); with O: bwd2_kernel<hd>
        for form, o_arg in (("out=None", None), ("out=O", out)):
            dqkv = torch.full_like(qkv, float("nan"))
            ops.attention_bwd(qkv, dout, lse, dqkv, out=o_arg, **kw)
            grads[form] = dqkv
    torch.cuda.synchronize()
    return out, lse, grads


@pytest.mark.parametrize("case", R.ATTN_CASES, ids=repr)
def test_attention_dropout(dev, case):
    out, lse, grads = run_case(dev, case)
    o_ref, lse_ref, g_ref = R.attn_case_reference(case)
    t_out, t_bwd, t_lse = R.attn_tols(case.dtype)
    e_out, e_lse = R.rel_err(out, o_ref), lse_err(lse, lse_ref)
    e_bwd = {f: R.rel_err(g, g_ref) for f, g in grads.items()}
    print(f"{case}: out {e_out:.3g} (<{t_out:g}), lse {e_lse:.3g} (<{t_lse:g}), dqkv {e_bwd} (<{t_bwd:g})")
    assert e_out < t_out and e_lse < t_lse
    for f, e in e_bwd.items():
        assert e < t_bwd, (f, e)


@pytest.mark.parametrize("case", R.HIDE0_CASES, ids=repr)
def test_attention_dropout_fully_masked_query(dev, case):
    """Key 0 of batch row 1 hidden under causal: its query 0 has no allowed key — out == 0, lse == -inf, dq == 0,
    nothing NaN, and every other row as the reference."""
    out, lse, grads = run_case(dev, case)
    o_ref, lse_ref, g_ref = R.attn_case_reference(case)
    t_out, t_bwd, t_lse = R.attn_tols(case.dtype)
    S, D = case.S, case.H * case.hd
    assert not torch.isnan(out).any()
    assert torch.all(out[S] == 0)
    assert torch.all(lse.view(case.B, case.H, S)[1, :, 0] == float("-inf"))
    e_out, e_lse = R.rel_err(out, o_ref), lse_err(lse, lse_ref)
    print(f"{case}: out {e_out:.3g}, lse {e_lse:.3g}")
    assert e_out < t_out and e_lse < t_lse
    for f, g in grads.items():
        assert not torch.isnan(g).any(), f
        assert torch.all(g[S, :D] == 0), f
        e = R.rel_err(g, g_ref)
        print(f"  {f}: dqkv {e:.3g}")
        assert e < t_bwd, (f, e)


def _packed_layout(lens, S, holes, dev):
    """Sequences of `lens` tokens in a launch of S: (seq_off, seq_len, padded key mask [B, S] on the host, packed key
    mask [B*S], live padded rows)."""
    B = len(lens)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    km = torch.zeros((B, S), dtype=torch.int32)
    for b, n in enumerate(lens):
        km[b, :n] = 1
    for b, t in holes:
        km[b, t] = 0
    rows = torch.cat([torch.arange(b * S, b * S + n) for b, n in enumerate(lens)])
    kmp = torch.zeros(B * S, dtype=torch.int32)
    kmp[: len(rows)] = km.reshape(-1)[rows]
    i32 = dict(dtype=torch.int32, device=dev)
    return torch.tensor(offs, **i32), torch.tensor(lens, **i32), km, kmp.to(dev), rows.to(dev)


def _packed_run(dev, dtype, H, hd, lens, S, desc, short_forms=(False,)):
    """The padded launch and the packed one(s) over the same tokens, dropout on; returns the padded (out, lse, dqkv),
    the packed ones per short_only form, the live rows and the fp64 reference (padded numbering)."""
    B, D = len(lens), H * hd
    so, sl, km, kmp, rows = _packed_layout(lens, S, [(3, 2), (5, 7)] if max(lens) > 32 else [(3, 2)], dev)
    n = len(rows)
    qkv = R.randn((B * S, 3 * D), 11).to(dev, dtype)
    dout = torch.zeros((B * S, D), dtype=dtype, device=dev)  # dead rows feed no loss
    dout[rows] = R.randn((n, D), 12).to(dev, dtype)
    drop = dev_drop(desc, dev)
    kw = dict(B=B, S=S, H=H, hd=hd, scale=hd ** -0.5, causal=True, drop=drop)
    o_pad = torch.zeros((B * S, D), dtype=dtype, device=dev)
    lse_pad = torch.full((B * H * S,), 7.0, device=dev)
    ops.attention_fwd(qkv, o_pad, key_mask=km.to(dev), lse=lse_pad, **kw)
    d_pad = torch.zeros_like(qkv)
    ops.attention_bwd(qkv, dout, lse_pad, d_pad, key_mask=km.to(dev), out=o_pad, **kw)
    qkv_c, dout_c = torch.zeros_like(qkv), torch.zeros_like(dout)
    qkv_c[:n], dout_c[:n] = qkv[rows], dout[rows]
    packed = {}
    for short in short_forms:
        o = torch.zeros((B * S, D), dtype=dtype, device=dev)
        lse = torch.full((B * H * S,), 7.0, device=dev)
        ops.attention_fwd(qkv_c, o, key_mask=kmp, lse=lse, seqs=(so, sl), short_only=short, **kw)
        d = torch.zeros_like(qkv_c)
        ops.attention_bwd(qkv_c, dout_c, lse, d, key_mask=kmp, out=o, seqs=(so, sl), short_only=short, **kw)
        packed[short] = (o, lse, d)
    torch.cuda.synchronize()
    keep = R.attn_keep(desc[0], B, H, S, desc[1])
    ref = R.attn_reference(qkv.cpu(), dout.cpu(), B, S, H, hd, hd ** -0.5, True, km, keep, desc[0].p)
    return (o_pad, lse_pad, d_pad), packed, rows, ref


def _live_lse(lse, lens, B, H, S):
    return torch.cat([lse.view(B, H, S)[b, :, :n].reshape(-1) for b, n in enumerate(lens)])


@pytest.mark.parametrize("dtype,H,hd,big", [(torch.bfloat16, 2, 64, False), (torch.float32, 2, 32, True)])
def test_attention_packed_equals_padded_with_dropout(dev, dtype, H, hd, big):
    """include/icap.h icap_attn_args: a packed launch keeps the padded [B, H, S, S] dropout numbering, so it equals
    the padded launch bitwise on the live rows with dropout on (fwd2 / bwd2 in their short and long passes, and the
    VALU kernels); both are the fp64 reference with that numbering."""
    lens, S = [1, 16, 17, 32, 33, 65], 65
    B = len(lens)
    desc = R.make_desc(0.1, big)
    (o_pad, lse_pad, d_pad), packed, rows, (o_ref, lse_ref, g_ref) = _packed_run(dev, dtype, H, hd, lens, S, desc)
    o_pk, lse_pk, d_pk = packed[False]
    n = len(rows)
    assert torch.equal(o_pk[:n], o_pad[rows])
    assert torch.equal(d_pk[:n], d_pad[rows])
    assert torch.equal(_live_lse(lse_pk, lens, B, H, S), _live_lse(lse_pad, lens, B, H, S))
    t_out, t_bwd, t_lse = R.attn_tols(dtype)
    rc = rows.cpu()
    e = (R.rel_err(o_pad, o_ref), R.rel_err(d_pad, g_ref), R.rel_err(o_pk[:n], o_ref[rc]),
         R.rel_err(d_pk[:n], g_ref[rc]), lse_err(_live_lse(lse_pk, lens, B, H, S), _live_lse(lse_ref, lens, B, H, S)))
    print(f"packed/padded vs fp64: padded out {e[0]:.3g} dqkv {e[1]:.3g}; packed out {e[2]:.3g} dqkv {e[3]:.3g} "
          f"lse {e[4]:.3g}")
    assert e[0] < t_out and e[2] < t_out and e[1] < t_bwd and e[3] < t_bwd and e[4] < t_lse


def test_attention_short_only_equals_both_passes_with_dropout(dev):
    """Every packed sequence <= 32 tokens in a launch of S = 65 (the benchmark's GPT-2 attention form): the short pass
    alone stores what the two passes store, bitwise, with dropout on — and that is the fp64 reference."""
    lens, S, H, hd = [1, 16, 17, 32, 5, 31], 65, 2, 64
    B = len(lens)
    desc = R.make_desc(0.1, True)
    _, packed, rows, (o_ref, lse_ref, g_ref) = _packed_run(dev, torch.bfloat16, H, hd, lens, S, desc, (False, True))
    for a, b in zip(packed[False], packed[True]):
        assert torch.equal(a, b)
    o, lse, d = packed[True]
    n, rc = len(rows), rows.cpu()
    t_out, t_bwd, t_lse = R.attn_tols(torch.bfloat16)
    e = (R.rel_err(o[:n], o_ref[rc]), R.rel_err(d[:n], g_ref[rc]),
         lse_err(_live_lse(lse, lens, B, H, S), _live_lse(lse_ref, lens, B, H, S)))
    print(f"short_only vs fp64: out {e[0]:.3g} dqkv {e[1]:.3g} lse {e[2]:.3g}")
    assert e[0] < t_out and e[1] < t_bwd and e[2] < t_lse


# ------------------------------------------------------------------------------------------------ GEMM epilogue


def _c_buf(case, dev):
    """The output and, for a strided case, the [M, ldc] buffer it is a view of (sentinel 7 past column N)."""
    if case.ldc is None:
        return torch.empty((case.M, case.N), device=dev, dtype=case.dtype), None
    full = torch.full((case.M, case.ldc), 7.0, device=dev, dtype=case.dtype)
    return full[:, : case.N], full


class _KernelNames:
    """ops.GEMM_TIMER stand-in: records the kernel instantiation each launch resolves to, and runs it."""

    def __init__(self):
        self.names = []

    def launch(self, key, flops, fn):
        self.names.append(key[0])
        fn()


@pytest.mark.parametrize("case", R.GEMM_CASES, ids=repr)
def test_gemm_epilogue_dropout(dev, case, monkeypatch):
    """include/icap.h icap_gemm epilogue order with dropout: C = keep * act(A B^T + bias) / (1 - p) + resid with aux
    taken before the mask and the mask index offset + row*N + col (N, not ldc); backward
    dZ = alpha * acc * keep / (1 - p) * act'(aux) regenerating the forward's mask from the same descriptor."""
    t = {k: v.to(dev) for k, v in case.inputs().items()}
    drop, keep, tol = dev_drop(case, dev), R.gemm_keep(case), R.gemm_tol(case.dtype)
    M, N = case.M, case.N
    sk = dict(split_k=case.split_k)
    rec = _KernelNames()
    monkeypatch.setattr(ops, "GEMM_TIMER", rec)
    C1, full1 = _c_buf(case, dev)
    ops.gemm(t["A"], t["B"], C1, bias=t["bias"], resid=t["resid"], drop=drop, **sk)         # GPT-2 ra / rm
    C2, full2 = _c_buf(case, dev)
    aux = torch.empty((M, N), device=dev, dtype=case.dtype)
    ops.gemm(t["A"], t["B"], C2, bias=t["bias"], act=L.ACT_RELU, aux=aux, drop=drop, **sk)  # the mapper's dff
    dZ, full3 = _c_buf(case, dev)
    ops.gemm(t["G"], t["W"], dZ, dact=L.ACT_RELU, dact_src=aux, drop=drop, alpha=R.BWD_ALPHA, **sk)
    torch.cuda.synchronize()
    ref = R.gemm_reference(case, keep, aux=aux)
    e = dict(resid=R.rel_err(C1, ref["resid"]), aux=R.rel_err(aux, ref["z"]), relu=R.rel_err(C2, ref["relu"]),
             dz=R.rel_err(dZ, ref["dz"]))
    print(f"{case}: " + ", ".join(f"{k} {v:.3g}" for k, v in e.items()) + f" (<{tol:g})")
    print("  kernels (resid, relu + aux, dact):", rec.names)
    assert max(e.values()) < tol, e
    assert len(rec.names) == 3 and all(("skinny" in n) == case.name.startswith("skinny") for n in rec.names)
    # the zero pattern, exactly: a dropped element is resid / 0 / 0; a kept one of some size is not
    C1c, C2c, dZc, rs = C1.cpu(), C2.cpu(), dZ.cpu(), t["resid"].cpu()
    z = ref["z"]
    assert torch.all((C1c == rs)[~keep]) and torch.all(C2c[~keep] == 0) and torch.all(dZc[~keep] == 0)
    assert torch.all((C1c != rs)[keep & (z.abs() > 0.02 + 2.0 ** -6 * rs.double().abs())])
    assert torch.all(C2c[keep & (z > 0.02)] > 0)
    acc = t["G"].double().cpu() @ t["W"].double().cpu().t()
    assert torch.all(dZc[keep & (aux.cpu() > 0) & (acc.abs() > 1e-3)] != 0)
    for full in (full1, full2, full3):
        if full is not None:
            assert torch.all(full[:, N:] == 7.0)


# ------------------------------------------------------------------------------------------------ layernorm_bwd


@pytest.mark.parametrize("case", R.LN_CASES, ids=repr)
def test_layernorm_bwd_dx_drop(dev, case):
    """icap_layernorm_bwd's fused residual-dropout output (the backward of every GPT-2 / mapper block's residual
    dropout): dx_drop = dx * keep(offset + r*D + c) / (1 - p) beside dx = LN'(x)^T dy (+ dres)."""
    t = {k: (None if v is None else v.to(dev)) for k, v in case.inputs().items()}
    rows, D = case.rows, case.D
    n = rows if case.rows_dev is None else case.rows_dev
    x, g, b = t["x"], t["gamma"], t["beta"]
    y = torch.empty_like(x)
    mean, rstd = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
    ops.layernorm_fwd(x, g, b, 1e-5, y, mean, rstd)
    dx, dxd = torch.full_like(x, 7.0), torch.full_like(x, 7.0)
    dg = db = ws = None
    if case.params:
        dg, db = torch.zeros(D, device=dev), torch.zeros(D, device=dev)
        ws = torch.empty(ops.layernorm_bwd_workspace(rows, D), dtype=torch.uint8, device=dev)
    rdev = None if case.rows_dev is None else torch.tensor([n], dtype=torch.int32, device=dev)
    ops.layernorm_bwd(x, g, mean, rstd, t["dy"], dx, dres=t["dres"], dx_drop=dxd, drop=dev_drop(case, dev),
                      dgamma=dg, dbeta=db, workspace=ws, dy_rowmap=t["rowmap"], rows_dev=rdev)
    torch.cuda.synchronize()
    keep = R.ln_keep(case)
    gx, gxd, gg, gb = R.ln_reference(case, keep)
    t_dx, t_dg, t_db = R.ln_tols(case.dtype)
    e_dx, e_dxd = R.rel_err(dx[:n], gx), R.rel_err(dxd[:n], gxd)
    msg = f"{case}: dx {e_dx:.3g}, dx_drop {e_dxd:.3g} (<{t_dx:g})"
    assert e_dx < t_dx and e_dxd < t_dx, msg
    # the zero pattern is the mask's, exactly (a row whose dy the row map zeroes has dx == 0 itself without dres)
    assert torch.equal(dxd[:n].cpu() == 0, ~keep[:n] | (gx == 0))
    assert torch.all(dx[n:] == 7.0) and torch.all(dxd[n:] == 7.0)  # rows past rows_dev untouched in both outputs
    if case.params:
        e_dg, e_db = R.rel_err(dg, gg), R.rel_err(db, gb)
        msg += f", dgamma {e_dg:.3g} (<{t_dg:g}), dbeta {e_db:.3g} (<{t_db:g})"
        assert e_dg < t_dg and e_db < t_db, msg
    print(msg)
