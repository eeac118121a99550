"""The references of tests/decode_refs.py against independent definitions, on the CPU: what
test_decode_kernels_gpu.py measures the kernels with has to be right on its own first."""

import math

import pytest
import torch

from decode_refs import (argmax_ref, decode_ref, gather_cache, greedy_bookkeeping, greedy_chunk, identity_anc,
                         random_anc, special_rows)
from test_kernels_gpu import ref_attention


def _cache(T, B, D, pad, seed):
    g = torch.Generator().manual_seed(seed)
    full = torch.full((T * B, 3 * D + pad), float("nan"), dtype=torch.float64)
    full[:, : 3 * D] = torch.randn((T * B, 3 * D), generator=g, dtype=torch.float64)
    return full


@pytest.mark.parametrize("pos", [0, 7, 19])
@pytest.mark.parametrize("B,H,hd,pad", [(3, 3, 64, 8), (2, 2, 32, 0)])
def test_decode_ref_is_last_row_of_causal_attention(B, H, hd, pos, pad):
    T, D, scale = 20, H * hd, 1.0 / math.sqrt(hd)
    full = _cache(T, B, D, pad, seed=1)
    out, absw = decode_ref(full[:, : 3 * D], B, H, hd, pos, scale)
    x = full[:, : 3 * D].view(T, B, 3, H, hd).permute(2, 1, 3, 0, 4)  # [3, B, H, T, hd]
    o = ref_attention(x[0], x[1], x[2], scale, True, None)[:, :, pos]
    assert (out - o.reshape(B, D)).abs().max().item() < 1e-12
    # absw: the same weights over |v|, so it bounds |out| and is what plain attention over |v| gives
    oa = ref_attention(x[0], x[1], x[2].abs(), scale, True, None)[:, :, pos]
    assert (absw - oa.reshape(B, D)).abs().max().item() < 1e-12
    assert (out.abs() <= absw + 1e-15).all()


@pytest.mark.parametrize("pos", [0, 8, 19])
def test_decode_ref_ancestry_is_a_physical_gather(pos):
    B, H, hd, T = 3, 3, 64, 20
    D = H * hd
    full = _cache(T, B, D, 8, seed=2)
    cache = full[:, : 3 * D]
    anc = random_anc(pos, B, seed=3 + pos)
    a, aw = decode_ref(cache, B, H, hd, pos, 0.125, anc)
    g, gw = decode_ref(gather_cache(cache, B, D, pos, anc), B, H, hd, pos, 0.125)
    # (fp64 rounding only: the two calls hand einsum differently laid-out operands)
    assert (a - g).abs().max().item() < 1e-13 and (aw - gw).abs().max().item() < 1e-13
    i, _ = decode_ref(cache, B, H, hd, pos, 0.125, identity_anc(pos, B))
    n, _ = decode_ref(cache, B, H, hd, pos, 0.125)
    assert (i - n).abs().max().item() < 1e-13
    if pos:  # the table really moves rows: the gathered cache differs and so does the result
        assert not torch.equal(anc, identity_anc(pos, B))
        assert not torch.equal(a, n)


def test_random_anc_shape_and_last_row():
    anc = random_anc(129, 3, seed=5)
    assert anc.dtype == torch.int32 and tuple(anc.shape) == (130, 3)
    assert anc.min().item() == 0 and anc.max().item() == 2
    assert anc[129].tolist() == [0, 1, 2]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V,ld", [(50257, 50304), (50, 56), (64, 72), (65, 72), (70001, 70008)])
def test_argmax_ref_reproduces_hand_written_winners(V, ld, dtype):
    lg, names, winners = special_rows(V, ld, dtype)
    assert argmax_ref(lg[:, :V]).tolist() == winners.tolist(), names
    # the padding really is poisoned: over the whole row the answer would be a padding column
    whole = argmax_ref(lg)
    assert all(w >= V for w, n in zip(whole.tolist(), names) if n != "two_nans")
    pad = lg[:, V:].float()
    assert pad.isnan().any(dim=1).all() and pad.isinf().any(dim=1).all()
    for must in ("first", "last", "tie_chunk_edge", "two_nans", "plus_inf", "all_minus_inf", "padding"):
        assert must in names


def test_special_rows_indices_at_gpt2_vocabulary():
    V = 50257
    assert greedy_chunk(V) == 6288
    _, names, winners = special_rows(V, 50304, torch.bfloat16)
    w = dict(zip(names, winners.tolist()))
    assert w["vector_end"] == 50255 and w["scalar_tail"] == 50256
    assert w["chunk_end"] == 6287 and w["chunk_start"] == 6288 and w["tie_chunk_edge"] == 6287
    assert w["tie_far"] == 5 and w["two_nans"] == 6291 and w["all_minus_inf"] == 0


def test_greedy_bookkeeping():
    eos = 9
    am = torch.tensor([4, 9, 2, 7])
    fin = torch.tensor([0, 0, 1, 0], dtype=torch.int32)
    tok, f = greedy_bookkeeping(am, fin, eos)
    assert tok.tolist() == [4, 9, 9, 7] and f.tolist() == [0, 1, 1, 0]
    tok, f = greedy_bookkeeping(am, fin, eos, forced=torch.tensor([9, 1, 3, 5]))
    assert tok.tolist() == [9, 1, 9, 5] and f.tolist() == [1, 0, 1, 0]
    assert fin.tolist() == [0, 0, 1, 0] and am.tolist() == [4, 9, 2, 7]  # inputs untouched
