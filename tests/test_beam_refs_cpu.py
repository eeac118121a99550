"""The host restatement of the beam state (tests/beam_refs.py) against transformers, before it judges a kernel:
driven with the oracle's own fp32 logits it must return the ids of tests/golden/beam4.npz (transformers' beam
search) and, at other widths / length penalties, the oracle's beam_generate."""

import os

import numpy as np
import pytest
import torch

from oracle import icap_oracle as O

import beam_refs as BR
from test_beam import TINY, _sd

GOLD = os.path.join(os.path.dirname(__file__), "golden", "beam4.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@torch.no_grad()
def ref_generate(sd, gcfg, prefix, L, W, lp=1.0):
    """Beam search by the restatement over O.gpt2_forward logits (full recompute per step, like the oracle)."""
    B, P, D = prefix.shape
    V = gcfg.vocab_size
    wte = sd["transformer.wte.weight"]
    ref = BR.BeamRef(B, W, V, L, P + L, gcfg.eos, lp)
    ref.init(P)
    for s in range(L):
        rows = [torch.cat((prefix[b].float(), wte[torch.from_numpy(ref.run_seq[b, i, :s].astype(np.int64))].float()))
                for b in range(B) for i in range(W)]
        _, logits = O.gpt2_forward(sd, gcfg, torch.stack(rows))
        val, idx, m, ls = BR.rowtop_ref(logits[:, -1, :V].float().numpy(), V, ref.K)
        ref.update(val, idx, m.astype(np.float32), ls.astype(np.float32), s, P + s - 1)
        if ref.done.all():
            break
    return ref.result()


@pytest.mark.parametrize("tag,scale,L", [("tiny", 1.0, 20), ("tiny", 4.0, 20), ("tiny", 5.0, 20), ("tiny", 6.0, 20),
                                         ("small", 4.0, 12)])
def test_restatement_matches_transformers(gold, tag, scale, L):
    gcfg, sd = _sd(tag, scale)
    ids = ref_generate(sd, gcfg, torch.from_numpy(gold[f"{tag}_prefix"]), L, 4)
    exp = gold[f"{tag}_s{scale:g}_ids"]
    assert ids.shape == exp.shape and np.array_equal(ids, exp), (ids, exp)


@pytest.mark.parametrize("W,lp", [(2, 1.0), (3, 0.5), (6, 2.0), (8, 1.0)])
def test_restatement_matches_oracle_widths(gold, W, lp):
    gcfg, sd = _sd("tiny", 5.0)
    prefix = torch.from_numpy(gold["tiny_prefix"])
    exp = O.beam_generate(sd, gcfg, prefix, 12, num_beams=W, length_penalty=lp).numpy()
    ids = ref_generate(sd, gcfg, prefix, 12, W, lp)
    assert ids.shape == exp.shape and np.array_equal(ids, exp), (W, lp, ids, exp)


def test_rowtop_ref_tie_order_and_tail():
    x = np.full((2, 40), 0.25, dtype=np.float32)
    x[1, 7] = 1.0
    val, idx, m, ls = BR.rowtop_ref(x, 37, 8)
    assert idx[0].tolist() == list(range(8)) and idx[1].tolist() == [7, 0, 1, 2, 3, 4, 5, 6]
    assert val[1].tolist() == [1.0] + [0.25] * 7
    assert m.tolist() == [0.25, 1.0] and abs(ls[0] - np.log(37.0)) < 1e-12
    val, idx, m, ls = BR.rowtop_ref(x, 3, 8)  # V < K: the tail is -inf / 0x7fffffff
    assert idx[0].tolist() == [0, 1, 2] + [BR.PAD_IDX] * 5 and bool(np.isneginf(val[0, 3:]).all())


def test_restatement_frozen_after_done_and_fallback():
    """Two hand-made captions at W = 2: one finishes both slots at step 1 and is done (its finished list never
    changes again, its running beams do); the other never sees EOS and finalises to running beam 0."""
    W, V, L, K, eos = 2, 16, 6, 8, 9
    ref = BR.BeamRef(2, W, V, L, 4 + L, eos, 0.0, K)
    ref.init(4)
    z = np.zeros(4, dtype=np.float32)

    def tables(rows):
        val = np.array([[v for v, _ in r] for r in rows], dtype=np.float32)
        idx = np.array([[t for _, t in r] for r in rows], dtype=np.int32)
        return val, idx

    plain = [(-0.5 * k, k) for k in range(K)]                      # tokens 0..7, no EOS
    eosy = [(0.0, eos)] + [(-4.0 - k, k) for k in range(K - 1)]   # EOS on top, the rest far below
    ref.update(*tables([plain, plain, plain, plain]), z, z, 0, 3)
    info = ref.update(*tables([eosy, eosy, plain, plain]), z, z, 1, 4)
    assert info[0]["new"] == [0, 1] and info[0]["done_now"] and ref.fin_cnt.tolist() == [2, 0]
    kept = (ref.fin_score.copy(), ref.fin_seq.copy(), ref.fin_len.copy())
    before = ref.run_seq.copy()
    info = ref.update(*tables([eosy, eosy, plain, plain]), z, z, 2, 5)
    assert info[0]["was_done"] and info[0]["hits"][0] and not info[0]["new"]
    assert np.array_equal(kept[0][0], ref.fin_score[0]) and np.array_equal(kept[1][0], ref.fin_seq[0])
    assert np.array_equal(kept[2][0], ref.fin_len[0]) and not np.array_equal(before[0], ref.run_seq[0])
    out, n = ref.finalize()
    assert n.tolist() == [2, L] and out[0].tolist() == [0, eos] + [eos] * (L - 2)
    assert out[1].tolist() == [0, 0, 0] + [eos] * (L - 3)
