"""tests/attn_refs.py on its own, without a GPU: the references against autograd of the plain fp64 definition, the
emulated rounding of each arithmetic family against every bound (worst ratio per output and family printed), the
reference-side mutants the bounds must reject — with the old whole-tensor rel_err limits shown to accept the two
that motivated this module — and the dispatch table: which kernel every GPU case reaches."""

import math

import pytest
import torch

import attn_refs as A
import dropout_refs as R

ALL = A.CASES + A.DROP_CASES + A.PACKED_CASES


def _plain(case):
    """autograd of the textbook definition: softmax over masked_fill(-inf) scores, dead rows zeroed."""
    qkv, dout = case.inputs()
    B, S, H, hd = case.B, case.S, case.H, case.hd
    x = qkv.double().view(B, S, 3, H, hd).permute(2, 0, 3, 1, 4).detach().requires_grad_(True)
    allowed = R.allowed_mask(B, S, case.causal, case.key_mask())
    s = ((x[0] @ x[1].transpose(-1, -2)) * case.scale).masked_fill(~allowed, float("-inf"))
    dead = ~allowed.any(-1, keepdim=True)
    pr = torch.softmax(s.masked_fill(dead, 0.0), -1).masked_fill(dead, 0.0)
    if case.keep is not None:
        pr = pr * case.keep * R.inv_keep(case.p)
    o = A.rows(pr @ x[2])
    (gx,) = torch.autograd.grad(o, x, dout.double())
    g = gx.permute(1, 3, 0, 2, 4).reshape(B * S, -1)
    D = H * hd
    return dict(out=o.detach(), lse=torch.logsumexp(s.detach(), -1).reshape(-1), dq=g[:, :D], dk=g[:, D:2 * D],
                dv=g[:, 2 * D:])


@pytest.mark.parametrize("case", ALL, ids=repr)
def test_references_equal_autograd(case):
    ref, pl = A.reference(case), _plain(case)
    qkv, dout = case.inputs()
    cf = A.intermediates(qkv, dout, case.B, case.S, case.H, case.hd, case.scale, case.causal, case.key_mask(),
                         case.keep, case.p)
    for k in A.OUTPUTS:
        for other in (pl[k], cf[k]):
            assert torch.equal(torch.isinf(ref[k]), torch.isinf(other)), k
            fin = ~torch.isinf(ref[k])
            if fin.any():
                tol = 1e-11 * max(1.0, ref[k][fin].abs().max().item())
                assert (ref[k][fin] - other[fin]).abs().max().item() <= tol, k
        assert (ref["A_" + k] >= 0).all()
        if k != "lse":  # the weight dominates the value, so A = 0 forces ref = 0 (the exact-zero elements)
            assert (ref[k].abs() <= ref["A_" + k] * (1 + 1e-12) + 1e-300).all(), k
    km, S, D = case.key_mask(), case.S, case.H * case.hd
    if km is not None:  # masked keys: dK = dV = 0 with a zero bound; fully masked queries: out = dQ = 0, lse = -inf
        dead_k = (km == 0).reshape(-1)
        for k in ("dk", "dv"):
            assert (ref[k][dead_k] == 0).all() and (ref["A_" + k][dead_k] == 0).all()
        dead_q = ~R.allowed_mask(case.B, S, case.causal, km).any(-1).reshape(case.B, S)  # [B, S]
        for k in ("out", "dq"):
            assert (ref[k][dead_q.reshape(-1)] == 0).all() and (ref["A_" + k][dead_q.reshape(-1)] == 0).all()
        lse = ref["lse"].view(case.B, case.H, S)
        assert torch.equal(lse == float("-inf"), dead_q[:, None, :].expand(case.B, case.H, S))


def test_emulation_meets_every_bound():
    worst, bad = {}, []
    for case in ALL:
        ref = A.reference(case)
        for form in (case.forms or ("O",)):
            got = A.emulate(case, form)
            if not case.forms:
                got = {k: got[k] for k in ("out", "lse")}
            for k, r in A.ratios(case.family, got, ref, form=form).items():
                fam = case.family + ("_O" if form == "O" and k in ("dq", "dk") and case.family == "mfma" else "")
                if not r <= 1.0:
                    bad.append((case.name, form, k, r))
                if r > worst.get((fam, k), (-1.0, ""))[0]:
                    worst[(fam, k)] = (r, case.name)
    for (fam, k), (r, name) in sorted(worst.items()):
        print(f"emulation worst ratio {fam:22s} {k:4s} {r:.3f}  ({name})")
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ mutants


def _suite_ref(B, S, H, hd, causal, km, big=False, allowed=None):
    """intermediates() on test_kernels_gpu.py test_attention's inputs (randn seeds 20 / 21, bf16)."""
    D = H * hd
    qkv = R.randn((B * S, 3 * D), 20)
    if big:
        qkv[:, :2 * D] *= 3
    qkv, dout = qkv.to(A.bf), R.randn((B * S, D), 21).to(A.bf)
    return A.intermediates(qkv, dout, B, S, H, hd, 1.0 / math.sqrt(hd), causal, km, None, 0.0, allowed=allowed)


def _dqkv(r):
    return torch.cat([r["dq"], r["dk"], r["dv"]], 1)


@pytest.mark.parametrize("S,causal,old_accepts", [(65, True, True), (257, False, False)])
def test_bounds_reject_a_dropped_key(S, causal, old_accepts):
    """The last query loses its last allowed key (an off-by-one at a tile edge), B = 2, H = 2, hd 64. At S = 65
    causal — the benchmark's GPT-2 form — the old limits (out rel_err < 1e-2, lse within 2e-2) accept it."""
    B, H, hd = 2, 2, 64
    ref = _suite_ref(B, S, H, hd, causal, None)
    allowed = R.allowed_mask(B, S, causal, None).clone()
    allowed[:, :, S - 1, S - 1] = False
    mut = _suite_ref(B, S, H, hd, causal, None, allowed=allowed)
    r = A.ratio(mut["out"], ref["out"], ref["A_out"], A.BOUNDS["mfma"]["out"])
    old_out, old_lse = R.rel_err(mut["out"], ref["out"]), (mut["lse"] - ref["lse"]).abs().max().item()
    print(f"dropped key S={S}: per-element ratio {r:.2f}; old out rel_err {old_out:.4f} (<1e-2), lse {old_lse:.4f} (<2e-2)")
    assert r > 1.0
    assert A.ratio(mut["lse"], ref["lse"], ref["A_lse"], A.BOUNDS["mfma"]["lse"], lse=True) > 1.0
    assert (old_out < 1e-2 and old_lse < 2e-2) == old_accepts


@pytest.mark.parametrize("S,big,masked,old_accepts", [(65, True, True, True), (128, False, False, None)])
def test_bounds_reject_zeroed_dk_rows(S, big, masked, old_accepts):
    """dK of the last three keys zeroed, causal, B = 2, H = 2, hd 64 (S = 65: batch row 0 masked from key 30 as in
    test_attention, row 1 whole so its late keys are live; q and k scaled by 3). Late keys under a causal mask have
    small gradients: the old dqkv rel_err < 2e-2 accepts S = 65 (0.018) and sits on the limit at S = 128 (0.0206;
    printed, not pinned)."""
    B, H, hd = 2, 2, 64
    km = None
    if masked:
        km = torch.ones((B, S), dtype=torch.int32)
        km[0, 30:] = 0
    ref = _suite_ref(B, S, H, hd, True, km, big=big)
    dk = ref["dk"].clone()
    dk.view(B, S, -1)[:, S - 3:] = 0
    r = A.ratio(dk, ref["dk"], ref["A_dk"], A.BOUNDS["mfma_O"]["dk"])
    old = R.rel_err(torch.cat([ref["dq"], dk, ref["dv"]], 1), _dqkv(ref))
    print(f"zeroed dK rows S={S}: per-element ratio {r:.2f}; old dqkv rel_err {old:.4f} (<2e-2)")
    assert r > 1.0
    if old_accepts is not None:
        assert (old < 2e-2) == old_accepts


def _case(name):
    return next(c for c in A.CASES if c.name == name)


@pytest.mark.parametrize("family,name", [("mfma_O", "v2-64-S65-cm"), ("valu_f32", "valu-f32-64-S65-cm")])
def test_bounds_reject_small_mutants(family, name):
    case = _case(name)
    ref = A.reference(case)
    B, S, H, hd = case.B, case.S, case.H, case.hd
    b = A.BOUNDS[family]
    dq = ref["dq"].clone()
    dq[:, hd:2 * hd] *= 0.5  # head 1
    assert A.ratio(dq, ref["dq"], ref["A_dq"], b["dq"]) > 1.0
    dv = ref["dv"].clone()
    assert case.key_mask()[0, S - 1] == 0
    dv[S - 1, 5] = 1e-3      # a masked key of batch row 0
    assert A.ratio(dv, ref["dv"], ref["A_dv"], b["dv"]) == float("inf")
    assert A.ratio(ref["lse"] + 0.005, ref["lse"], ref["A_lse"], b["lse"], lse=True) > 1.0
    for k in A.OUTPUTS:      # and the reference itself passes
        assert A.ratio(ref[k], ref[k], ref["A_" + k], b[k], lse=k == "lse") == 0.0


# ------------------------------------------------------------------------------------------------ dispatch


def test_dispatch_table():
    """Every GPU case reaches the kernel its name says (attn_refs.select restates mfma_attention_ok, mfma_fwd2_ok,
    mfma_bwd2_ok, mfma_fwd3_ok and fwd_rows), and the cases reach every kernel of attn_refs.KERNELS."""
    reached = set()
    for c in A.CASES:
        sel = c.selected()
        assert sel == c.expect, (c.name, sel, c.expect)
        reached |= set(sel.values())
    assert set(A.KERNELS) <= reached, set(A.KERNELS) - reached
    assert reached <= set(A.KERNELS), reached - set(A.KERNELS)


def test_dispatch_edges():
    D = 3 * 96
    with_o = A.Launch(3 * D, D + A.PAD, D, 3 * D + A.PAD, out_given=True)
    no_o = A.Launch(3 * D, D + A.PAD, D, 3 * D + A.PAD, out_given=False)
    # hd 96 with O: bwd2_kernel<96> fits (115,840 B) where v1's image (165,376 B) does not; without O nothing does
    assert A.mfma_bwd_lds(113, 96) == 165376 > A.LDS_CAP and A.mfma_bwd2_lds(128, 96) == 115840
    for S in (113, 128):
        assert A.select(A.bf, 96, S, with_o, True) == "bwd2_kernel<96>"
        assert A.select(A.bf, 96, S, no_o, True) is None
    assert A.select(A.bf, 96, 112, no_o, True) == "bwd_kernel<96>"
    # the largest sequences: v3's LDS image, the VALU backward and the one-chunk VALU forward
    l64 = A.Launch(576, 200, 192, 584)
    assert A.select(A.bf, 64, 512, l64, False) == "fwd3_kernel<64>" and A.mfma_fwd3_lds(513, 64) > A.LDS_CAP
    assert A.select(A.bf, 96, 352, with_o, False) == "fwd3_kernel<96>" and A.mfma_fwd3_lds(353, 96) > A.LDS_CAP
    assert A.select(A.f32, 64, 92, l64, True) == "attn_bwd_kernel<float>" and A.select(A.f32, 64, 93, l64, True) is None
    assert A.fwd_rows(127, 64) == 127 and A.fwd_rows(128, 64) == 64
    assert A.fwd_rows(197, 64) == 32 and A.fwd_rows(257, 64) == 16
    # packed launches: two passes above 32 tokens unless short_only
    assert A.packed_passes(65, False) == ("short", "long") and A.packed_passes(65, True) == ("short",)
    assert A.packed_passes(32, False) == ("single",)
    for c in A.PACKED_CASES:
        assert max(c.lens) <= (32 if c.short_only else c.S)
