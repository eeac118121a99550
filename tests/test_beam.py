"""Beam-4 caption decode. The reference has greedy / top-p only (src/models.py:327-477), so
the definition is transformers' own beam search (GPT2LMHeadModel.generate(num_beams=4), HF/generation/
utils.py:3208-3540) run on the goldens' caption prefixes by tools/make_goldens.py golden_beam ->
tests/golden/beam4.npz. `eos_scale` multiplies wte[eos] so captions finish at different steps.

CPU: oracle.beam_generate == transformers' ids. GPU (-m gpu): the KV-cached HIP beam decode (icap_beam_* +
ancestry-indexed icap_attention_decode_anc) == the golden in fp32, eager and HIP-graph replay; the bf16 decode
replayed step by step on the host restatement of the beam state (tests/beam_refs.py; the kernels themselves are
pinned in test_beam_kernels_gpu.py); early_exit=False."""

import os

import numpy as np
import pytest
import torch

from oracle import icap_oracle as O

GOLD = os.path.join(os.path.dirname(__file__), "golden", "beam4.npz")
TINY = O.GPT2Cfg(n_layer=2, n_embd=128, n_head=2, vocab_size=512, n_positions=128, eos=511)
CASES = [("tiny", 1.0, 20), ("tiny", 4.0, 20), ("tiny", 5.0, 20), ("tiny", 6.0, 20), ("small", 4.0, 12),
         ("small", 3.0, 12)]


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _cfg(tag):
    return TINY if tag == "tiny" else O.GPT2Cfg()


def _sd(tag, scale):
    gcfg = _cfg(tag)
    sd = O.gpt2_state_dict(gcfg, 0)
    sd["transformer.wte.weight"] = sd["transformer.wte.weight"].clone()
    sd["transformer.wte.weight"][gcfg.eos] *= scale
    return gcfg, sd


@pytest.mark.parametrize("tag,scale,L", CASES)
def test_oracle_beam_matches_transformers(gold, tag, scale, L):
    gcfg, sd = _sd(tag, scale)
    ids = O.beam_generate(sd, gcfg, torch.from_numpy(gold[f"{tag}_prefix"]), L, num_beams=4)
    assert np.array_equal(ids.numpy(), gold[f"{tag}_s{scale:g}_ids"]), (ids, gold[f"{tag}_s{scale:g}_ids"])


def _device_gpt(tag, scale, dtype, dev):
    from icap import GPT2LMHeadModel
    from icap.gpt2 import GPT2Config

    gc, sd = _sd(tag, scale)
    cfg = GPT2Config(vocab_size=gc.vocab_size, n_positions=gc.n_positions, n_embd=gc.n_embd, n_layer=gc.n_layer,
                     n_head=gc.n_head, layer_norm_epsilon=gc.eps, eos_token_id=gc.eos)
    gpt = GPT2LMHeadModel(cfg)
    gpt.load_state_dict(sd, strict=False)
    return gpt.to(dev).core(dtype), gc, sd


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("tag,scale,L", CASES)
def test_device_beam_matches_transformers_fp32(dev, gold, tag, scale, L, graph):
    """fp32 parity mode: the KV-cached HIP beam search returns transformers' ids exactly (eager launches and
    HIP-graph chunk replay with the early exit)."""
    core, _, _ = _device_gpt(tag, scale, torch.float32, dev)
    core.graph_decode = graph
    prefix = torch.from_numpy(gold[f"{tag}_prefix"]).to(dev)
    ids = core.beam_decode(prefix, L, num_beams=4).cpu()
    exp = gold[f"{tag}_s{scale:g}_ids"]
    assert ids.shape == exp.shape and np.array_equal(ids.numpy(), exp), (ids, exp)
    if graph:  # a second replay of the captured graphs (state re-initialised inside chunk 0)
        assert np.array_equal(core.beam_decode(prefix, L, num_beams=4).cpu().numpy(), exp)


@pytest.mark.gpu
def test_device_beam_width_and_penalty_vs_oracle(dev, gold):
    """Other widths / length penalties against the oracle restatement (pinned above to transformers at W = 4)."""
    core, gc, sd = _device_gpt("tiny", 5.0, torch.float32, dev)
    prefix = torch.from_numpy(gold["tiny_prefix"])
    for W, lp in ((2, 1.0), (3, 0.5), (6, 2.0), (8, 1.0)):
        exp = O.beam_generate(sd, gc, prefix, 12, num_beams=W, length_penalty=lp)
        got = core.beam_decode(prefix.to(dev), 12, num_beams=W, length_penalty=lp).cpu()
        assert torch.equal(got, exp), (W, lp, got, exp)


@pytest.mark.gpu
def test_beam_rowtop_kernel(dev):
    """icap_beam_rowtop against torch: top-K logits (ties -> lower id) and the row log-sum-exp."""
    from icap import ops

    g = torch.Generator().manual_seed(3)
    V, Vp = 50257, 50304
    for dt in (torch.float32, torch.bfloat16):
        x = torch.randn((37, Vp), generator=g).to(dt)
        x[5, 100] = x[5, 200] = x[5].max() + 1  # a tie at the top: 100 first
        st = ops.BeamState(37, 4, V, 8, 16, 50256, 1.0, dev)
        st.set_embedding(dt, 8, 16, torch.zeros(1, device=dev), torch.zeros(1, device=dev), None)
        xd = x.to(dev)
        from icap._lib import call
        from icap.ops import _ld, _stream, dtype_code
        call("icap_beam_rowtop", dtype_code(dt), 37, V, xd.data_ptr(), _ld(xd), st.K, st.top_val.data_ptr(),
             st.top_idx.data_ptr(), st.top_m.data_ptr(), st.top_ls.data_ptr(), _stream())
        xf = x[:, :V].float()
        vals, idx = torch.sort(xf, dim=1, descending=True, stable=True)
        assert torch.equal(st.top_idx[:37].cpu().long(), idx[:, : st.K]), dt
        assert torch.equal(st.top_val[:37].cpu(), vals[:, : st.K])
        lse = torch.logsumexp(xf.double(), dim=1)
        got = st.top_m[:37].cpu().double() + st.top_ls[:37].cpu().double()
        assert (got - lse).abs().max().item() < 1e-5
        assert int(st.top_idx[5, 0]) == 100 and int(st.top_idx[5, 1]) == 200


@pytest.mark.gpu
def test_beam_bf16_small_agreement_and_batch(dev, gold):
    """bf16 (the benchmarked precision): agreement with transformers' fp32 ids at GPT-2 small (reported, bounded
    loosely: bf16 logits reorder near-tied candidates), and a 128-caption batch through the graph runner that
    is well-formed (EOS-padded after the first EOS) and identical between two replays."""
    core, _, _ = _device_gpt("small", 4.0, torch.bfloat16, dev)
    prefix = torch.from_numpy(gold["small_prefix"]).to(dev)
    ids = core.beam_decode(prefix, 12, num_beams=4).cpu().numpy()
    exp = gold["small_s4_ids"]
    n = min(ids.shape[1], exp.shape[1])
    agree = float((ids[:, :n] == exp[:, :n]).mean())
    print(f"bf16 beam-4 vs transformers fp32: token agreement {agree:.3f}")
    assert agree >= 0.5
    g = torch.Generator().manual_seed(9)
    big = (torch.randn((128, prefix.shape[1], prefix.shape[2]), generator=g) * float(prefix.float().std())).to(dev)
    a = core.beam_decode(big, 20, num_beams=4).cpu()
    b = core.beam_decode(big, 20, num_beams=4).cpu()
    assert torch.equal(a, b)
    eos = 50256
    for row in a:
        hit = (row == eos).nonzero()
        if hit.numel():
            assert bool((row[int(hit[0]):] == eos).all())


# ------------------------------------------------------------------------- the device's own steps, replayed
def _record_steps(monkeypatch, with_logits=False):
    """Wrap ops.BeamState.step: after each call keep (state, step, pos, top_val, top_idx, top_m, top_ls[, logits])
    as the device left them."""
    from icap import ops

    rec = []
    orig = ops.BeamState.step

    def step(self, logits, step, pos, x):
        orig(self, logits, step, pos, x)
        R = self.B * self.W
        rec.append((self, step, pos, self.top_val[:R].cpu().numpy(), self.top_idx[:R].cpu().numpy(),
                    self.top_m[:R].cpu().numpy(), self.top_ls[:R].cpu().numpy(),
                    logits[:R, : self.V].float().cpu() if with_logits else None))

    monkeypatch.setattr(ops.BeamState, "step", step)
    return rec


def _replay(rec, P, eos, lp=1.0, before=None):
    """The restatement (tests/beam_refs.py) driven by the recorded row tables; before(ref, record) runs ahead of
    each update."""
    import beam_refs as BR

    st = rec[0][0]
    ref = BR.BeamRef(st.B, st.W, st.V, st.max_len, st.T, eos, lp, st.K)
    ref.init(P)
    for r in rec:
        if before is not None:
            before(ref, r)
        ref.update(r[3], r[4], r[5], r[6], r[1], r[2])
    return ref


@pytest.mark.gpu
def test_beam_bf16_small_replay_exact(dev, gold, monkeypatch):
    """bf16 at the GPT-2 small geometry (the benchmarked precision): whatever the bf16 logits are, the beam
    bookkeeping on top of them is exact. The restatement replayed on the device's own row tables reproduces the
    device's ids, out_len, final running histories and KV ancestry; the graph runner returns the same ids."""
    import beam_refs as BR
    from icap import ops

    core, gc, _ = _device_gpt("small", 4.0, torch.bfloat16, dev)
    core.graph_decode = False
    prefix = torch.from_numpy(gold["small_prefix"]).to(dev)
    rec = _record_steps(monkeypatch)
    ids = core.beam_decode(prefix, 12, num_beams=4).cpu().numpy()
    monkeypatch.undo()
    assert [r[1] for r in rec] == list(range(len(rec))) and len(rec) >= 8
    st, pos = rec[0][0], rec[-1][2]
    ref = _replay(rec, prefix.shape[1], gc.eos)
    # no decision of this run hangs on the last bits of a powf: both sides of every finished-score comparison are
    # within 2 ulp of their exact quotients (a <= 1-ulp powf, one rounded divide), so 8 ulp apart cannot swap
    assert not ref.fragile_comparisons(rel=8 * 2.0 ** -23), ref.fragile_comparisons(rel=8 * 2.0 ** -23)[:3]
    out, n = ref.finalize()
    assert np.array_equal(st.out_len.cpu().numpy(), n), (st.out_len, n)
    assert np.array_equal(st.out.cpu().numpy(), out)
    assert np.array_equal(ids, ref.result()), (ids, ref.result())
    ws = BR.split_workspace(st.ws.cpu().numpy(), ops.beam_layout(st.B, st.W, st.T, st.max_len), st.B, st.W, st.T,
                            st.max_len)
    BR.assert_state_equal(ref, ws, rec[-1][1], pos, tag="small bf16")
    core.graph_decode = True
    assert np.array_equal(core.beam_decode(prefix, 12, num_beams=4).cpu().numpy(), ids)


@pytest.mark.gpu
def test_beam_bf16_rows_follow_their_histories(dev, gold, monkeypatch):
    """bf16, tiny geometry, tolerance-free: at every step >= 1, each row whose claimed history (the restatement's
    run_seq before the step) differs from all its siblings' must have produced logits nearer (L2) to the oracle's
    fp32 logits of its own history than to those of any sibling's. A wrong parent in the bf16 ancestry path reads
    a sibling's keys and lands on the sibling's logits."""
    core, gc, sd = _device_gpt("tiny", 5.0, torch.bfloat16, dev)
    core.graph_decode = False
    prefix = torch.from_numpy(gold["tiny_prefix"])
    rec = _record_steps(monkeypatch, with_logits=True)
    core.beam_decode(prefix.to(dev), 20, num_beams=4)
    monkeypatch.undo()
    wte = sd["transformer.wte.weight"]
    checked = [0]

    def before(ref, r):
        step, logits = r[1], r[7]
        if step == 0:
            return
        B, W = ref.B, ref.W
        hist = torch.from_numpy(ref.run_seq[:, :, :step].astype(np.int64))            # [B, W, step]
        rows = torch.cat((prefix.float().repeat_interleave(W, dim=0), wte[hist.reshape(B * W, step)].float()), dim=1)
        with torch.no_grad():
            _, ol = O.gpt2_forward(sd, gc, rows)
        ol = ol[:, -1, : gc.vocab_size].float().view(B, W, -1)
        for b in range(B):
            for i in range(W):
                if any(j != i and torch.equal(hist[b, j], hist[b, i]) for j in range(W)):
                    continue
                d = (ol[b] - logits[b * W + i][None, :]).norm(dim=1)
                assert int(d.argmin()) == i, (step, b, i, d.tolist())
                checked[0] += 1

    _replay(rec, prefix.shape[1], gc.eos, before=before)
    assert checked[0] >= 4 * len(rec)  # the check ran on most rows, not on a handful


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("scale", [1.0, 4.0, 5.0, 6.0])
def test_device_beam_fixed_work_same_ids(dev, gold, scale, graph):
    """early_exit=False (all max_length steps; finished captions stay frozen) returns the ids of the early-exit
    form, which are the golden's, in fp32 on the tiny cases, eager and graph."""
    core, _, _ = _device_gpt("tiny", scale, torch.float32, dev)
    core.graph_decode = graph
    prefix = torch.from_numpy(gold["tiny_prefix"]).to(dev)
    exp = gold[f"tiny_s{scale:g}_ids"]
    full = core.beam_decode(prefix, 20, num_beams=4, early_exit=False).cpu().numpy()
    early = core.beam_decode(prefix, 20, num_beams=4, early_exit=True).cpu().numpy()
    assert full.shape == exp.shape and np.array_equal(full, exp), (full, exp)
    assert np.array_equal(early, full)
