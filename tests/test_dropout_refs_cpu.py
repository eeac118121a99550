"""The references of tests/dropout_refs.py on the CPU: what test_dropout_sites_gpu.py and test_dropout_step_gpu.py
measure the kernels with has to be right, and able to tell a wrong mask from the right one, on its own first.

The discrimination tests evaluate every kernel-level reference, on the inputs the GPU tests use, with the mask of a
shifted offset and with the two mask indices swapped: the output and every gradient then move by more than 10x the
bound the GPU test holds the kernel to, so no bound there is vacuous.
"""

from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dropout_refs as R
from oracle import icap_oracle as O
from test_dropout_hash import keep_mask
from test_kernels_gpu import ref_attention

G = O.GPT2Cfg(n_layer=2, n_embd=128, n_head=2, vocab_size=512, n_positions=128, eos=511)   # test_model_gpu.TINY_G
M = O.MapperCfg(embed_dim=64, gpt_dim=128, prefix_length=5, hidden_length=4, num_layers=2)  # TINY_M


def fake_trainer(B, L, seed, counter, p=0.1):
    """What MaskedOracle reads of a CaptionTrainer, with the descriptors laid out by the cores' own drops()."""
    from icap.gpt2 import GPT2Core
    from icap.mapper import TransformerMapperCore

    ctr = torch.full((1,), counter, dtype=torch.int64)
    Sm, S = M.prefix_length + M.hidden_length, M.prefix_length + L
    mself = SimpleNamespace(S=Sm, D=M.gpt_dim, H=M.nhead)
    gself = SimpleNamespace(cfg=SimpleNamespace(embd_pdrop=p, attn_pdrop=p, resid_pdrop=p), D=G.n_embd, H=G.n_head)
    return SimpleNamespace(counter=ctr, mdr=TransformerMapperCore.drops(mself, True, p, seed, ctr, B),
                           gdr=GPT2Core.drops(gself, True, seed, ctr, B * S, B, S))


def batch(B=3, L=6, seed=1):
    return O.synthetic_batch(B, L, 4, G.vocab_size, G.eos, M.embed_dim, seed=seed)


def evaluate(msd, gsd, b, train, p):
    ids, mask, labels, emb = b
    prefix = O.mapper_forward(msd, M, emb.double(), train, p)
    loss, _ = O.caption_forward(gsd, G, prefix, ids, mask, labels, train, p)
    return loss


def val(loss):
    return float(loss.detach())


@pytest.fixture(scope="module")
def weights():
    msd = {k: v.double().requires_grad_(True) for k, v in O.mapper_state_dict(M, 0).items()}
    gsd = {k: v.double() for k, v in O.gpt2_state_dict(G, 0).items()}
    return msd, gsd


def test_masked_oracle_passes_through(weights):
    """train=False consumes no site and is the plain oracle; so is train=True with p -> tiny (threshold 0: every
    element kept, scale 1 / (1 - 1e-12))."""
    msd, gsd = weights
    b = batch()
    plain = evaluate(msd, gsd, b, False, 0.0)
    mo = R.MaskedOracle(fake_trainer(3, 6, 5, 1), M.num_layers, G.n_layer)
    with mo:
        off = evaluate(msd, gsd, b, False, 0.1)
    assert mo.calls == 0 and val(off) == val(plain)
    mo = R.MaskedOracle(fake_trainer(3, 6, 5, 1, p=1e-12), M.num_layers, G.n_layer)
    with mo:
        tiny = evaluate(msd, gsd, b, True, 1e-12)
    assert mo.calls == 4 * M.num_layers + 1 + 3 * G.n_layer
    assert abs(val(tiny) - val(plain)) < 1e-9
    assert O._drop.__module__ == O.__name__  # restored


def test_masked_oracle_is_a_function_of_its_descriptors(weights):
    msd, gsd = weights
    b = batch()
    res = {}
    for name, (seed, ctr) in {"a": (5, 1), "b": (5, 1), "counter": (5, 2), "seed": (6, 1)}.items():
        with R.MaskedOracle(fake_trainer(3, 6, seed, ctr), M.num_layers, G.n_layer):
            loss = evaluate(msd, gsd, b, True, 0.1)
            res[name] = (val(loss), torch.autograd.grad(loss, list(msd.values())))
    assert res["a"][0] == res["b"][0] and all(torch.equal(x, y) for x, y in zip(res["a"][1], res["b"][1]))
    plain = val(evaluate(msd, gsd, b, False, 0.0))
    for other in ("counter", "seed"):
        assert res[other][0] != res["a"][0] and abs(res["a"][0] - plain) > 1e-6
        for k, x, y in zip(msd, res["a"][1], res[other][1]):  # another draw moves every tensor's gradient
            assert float((x - y).norm() / x.norm()) > 0.1, (other, k)


def test_masked_oracle_counts_its_sites(weights):
    msd, gsd = weights
    with pytest.raises(AssertionError, match="unconsumed"):
        with R.MaskedOracle(fake_trainer(3, 6, 5, 1), M.num_layers, G.n_layer + 1):
            evaluate(msd, gsd, batch(), True, 0.1)
    with pytest.raises(AssertionError, match="more dropout calls"):
        with R.MaskedOracle(fake_trainer(3, 6, 5, 1), M.num_layers, G.n_layer - 1):
            evaluate(msd, gsd, batch(), True, 0.1)
    assert O._drop.__module__ == O.__name__


def test_keep_rates_and_numbering():
    d = R.Desc(0.1, R.BIG_SEED, R.BIG_OFFSET)
    for k in (R.site_keep(d, (300, 768), 3), R.attn_keep(d, 3, 4, 65, 3)):
        n = k.numel()
        assert abs(k.double().mean().item() - 0.9) < 4 * np.sqrt(0.1 * 0.9 / n)
    # row-major numbering, the counter read from the descriptor's tensor, and the packed row map
    ctr = torch.full((1,), 3, dtype=torch.int64)
    dc = R.Desc(0.1, 99, 7, ctr)
    flat = torch.from_numpy(keep_mask(99, 7, 6 * 5 * 8, R.p32(0.1), 3))
    assert torch.equal(R.site_keep(dc, (6, 5, 8)).reshape(-1), flat)
    ak = R.attn_keep(dc, 2, 3, 5)
    for b, h, q, k in ((0, 0, 0, 1), (1, 2, 1, 3), (0, 2, 4, 0)):
        assert bool(ak[b, h, q, k]) == bool(flat[(b * 3 + h) * 25 + q * 5 + k])
    so, sl = [0, 3, 4], [3, 1, 5]
    rows = R.packed_rows(so, sl, 5)
    assert rows.tolist() == [0, 1, 2, -1, -1, 3, -1, -1, -1, -1, 4, 5, 6, 7, 8]
    pk = R.site_keep(dc, (3, 5, 8), rows=rows).reshape(15, 8)
    dense = R.site_keep(dc, (9, 8))
    for r, dr in enumerate(rows):
        assert torch.equal(pk[r], dense[dr]) if dr >= 0 else bool(pk[r].all())
    k = R.site_keep(dc, (3, 5, 8), rows=rows)[torch.from_numpy(rows.reshape(3, 5) >= 0)]
    assert abs(k.double().mean().item() - 0.9) < 4 * np.sqrt(0.09 / k.numel())


def test_ref_attention_drop_against_plain_definition():
    B, H, S, hd = 2, 3, 19, 8
    q, k, v = (R.randn((B, H, S, hd), s).double() for s in (1, 2, 3))
    km = torch.ones((B, S), dtype=torch.int32)
    km[0, 11:] = 0
    o, lse = R.ref_attention_drop(q, k, v, 0.3, True, km, None, 0.0)
    assert (o - ref_attention(q, k, v, 0.3, True, km)).abs().max().item() < 1e-12
    # with a mask: the explicit sum over kept keys
    keep = R.attn_keep(R.Desc(0.5, 3, 0), B, H, S)
    o, lse2 = R.ref_attention_drop(q, k, v, 0.3, True, km, keep, 0.5)
    s = torch.einsum("bhqd,bhkd->bhqk", q, k) * 0.3
    allowed = R.allowed_mask(B, S, True, km)
    w = torch.exp(s - lse[..., None]) * allowed * keep * 2.0
    assert (o - w @ v).abs().max().item() < 1e-12 and torch.equal(lse, lse2)
    # a query row with no allowed key: zeros and -inf, nothing NaN, zero gradient for that query
    km[1, 0] = 0
    qr = q.clone().requires_grad_(True)
    o, lse = R.ref_attention_drop(qr, k, v, 0.3, True, km, keep, 0.5)
    (gq,) = torch.autograd.grad(o, qr, torch.ones_like(o))
    assert not torch.isnan(o).any() and not torch.isnan(gq).any()
    assert torch.all(o[1, :, 0] == 0) and torch.all(lse[1, :, 0] == float("-inf")) and torch.all(gq[1, :, 0] == 0)
    assert torch.isfinite(lse[0]).all() and torch.isfinite(lse[1, :, 1:]).all()


def _moved(ref, wrong, bound, what):
    e = R.rel_err(wrong, ref)
    assert e > 10 * bound, (what, e, bound)
    return e


@pytest.mark.parametrize("case", R.ATTN_CASES + R.HIDE0_CASES, ids=repr)
@pytest.mark.parametrize("variant", ["offset+1", "swapped"])
def test_attention_reference_discriminates(case, variant):
    o, lse, g = R.attn_case_reference(case)
    o2, lse2, g2 = R.attn_case_reference(case, variant)
    t_out, t_bwd, _ = R.attn_tols(case.dtype)
    assert torch.equal(lse, lse2)  # lse does not see the mask
    _moved(o, o2, t_out, "out")
    if case.bwd:
        D = case.H * case.hd
        _moved(g, g2, t_bwd, "dqkv")
        for i, name in enumerate(("dq", "dk", "dv")):
            _moved(g[:, i * D:(i + 1) * D], g2[:, i * D:(i + 1) * D], t_bwd, name)


@pytest.mark.parametrize("case", R.GEMM_CASES, ids=repr)
def test_gemm_reference_discriminates(case):
    ref = R.gemm_reference(case, R.gemm_keep(case))
    for variant in ("offset+1", "swapped") + (("ld",) if case.ldc else ()):
        wrong = R.gemm_reference(case, R.gemm_keep(case, variant))
        for k in ("resid", "relu", "dz"):
            _moved(ref[k], wrong[k], R.gemm_tol(case.dtype), (variant, k))
    # the order act -> mask -> + resid: masking after the residual, or before the activation's bias, is told apart
    t = {k: v.double() for k, v in case.inputs().items()}
    keep, s = R.gemm_keep(case), R.inv_keep(case.p)
    _moved(ref["resid"], keep * (ref["z"] + t["resid"]) * s, R.gemm_tol(case.dtype), "mask after resid")
    _moved(ref["relu"], torch.relu(keep * (t["A"] @ t["B"].t()) * s + t["bias"]), R.gemm_tol(case.dtype),
           "mask before bias")


@pytest.mark.parametrize("case", R.LN_CASES, ids=repr)
def test_layernorm_reference_discriminates(case):
    dx, dxd, dg, db = R.ln_reference(case, R.ln_keep(case))
    tol = R.ln_tols(case.dtype)[0]
    for variant in ("offset+1", "swapped", "ld"):
        dx2, dxd2, dg2, db2 = R.ln_reference(case, R.ln_keep(case, variant))
        assert torch.equal(dx, dx2) and torch.equal(dg, dg2) and torch.equal(db, db2)  # only dx_drop sees the mask
        _moved(dxd, dxd2, tol, variant)
    # and the reference's dx is the plain LayerNorm backward (torch's own, through another route)
    t = case.inputs()
    if case.rows_dev is None and t["rowmap"] is None:
        x = t["x"].double().requires_grad_(True)
        y = torch.nn.functional.layer_norm(x, (case.D,), t["gamma"].double(), t["beta"].double(), 1e-5)
        (y * t["dy"].double()).sum().backward()
        want = x.grad + (t["dres"].double() if t["dres"] is not None else 0)
        assert (dx - want).abs().max().item() < 1e-12
