"""The kernels a bf16 caption runs through at decode time, each against an fp64 restatement of the same operation
(tests/decode_refs.py) at the sizes where its code takes another path: the two decode-attention kernels with and
without beam ancestry, the position-major prefill, the first-generation MFMA forward, every form of greedy_next,
and the glue kernels (add_position, gpt2_embed, embedding_scatter_add, l2norm_rows, convert, broadcast_rows,
sqnorm).

Tolerances. bf16 decode attention, per element: |got - ref| <= 2^-8 |ref| + 1e-4 absw with absw = sum_j p_j |v_j|:
one bf16 rounding of the fp32 result, plus fp32 accumulation and __expf ((n + hd + 16) 2^-24 < 2.5e-5 for
n <= 260; 1e-4 is the accumulation coefficient test_patch_embed_matches_conv uses). fp32: 1e-5 max|ref|, the
suite's fp32 attention tolerance. Wherever a kernel's arithmetic order cannot depend on addressing (ancestry,
padding, row order) the comparison is torch.equal.

Every pointer and stride here is one the dispatch accepts and the chosen kernel's vector loads are aligned for;
NaN sentinels are data the kernels must not read, never addresses.
"""

import functools
import math

import numpy as np
import pytest
import torch

from decode_refs import (argmax_ref, decode_ref, gather_cache, greedy_bookkeeping, greedy_chunk, identity_anc,
                         random_anc, special_rows)
from icap import ops
from test_dropout_hash import keep_mask
from test_kernels_gpu import ref_attention, rel_err

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
SENT = 777.0  # exact in bf16


# ------------------------------------------------------------------------------------------ decode attention
def _decode_data(B, H, hd, pos, dtype, seed=80):
    """Packed CPU cache values [(pos+2)*B, 3D] of `dtype` (N(0,1) per element; the row past pos is NaN), the case's
    random ancestry and the fp64 references (out, absw) without and with it. Computed once per case and shared;
    every call gets its own copies, so no test can change what another sees."""
    vals, anc, plain, with_anc = _decode_data_cached(B, H, hd, pos, dtype, seed)
    return vals.clone(), anc.clone(), tuple(t.clone() for t in plain), tuple(t.clone() for t in with_anc)


@functools.lru_cache(maxsize=None)
def _decode_data_cached(B, H, hd, pos, dtype, seed):
    D = H * hd
    g = torch.Generator().manual_seed(seed + 1000 * hd + pos)
    vals = torch.randn(((pos + 2) * B, 3 * D), generator=g)
    vals[(pos + 1) * B:] = NAN
    vals = vals.to(dtype)
    anc = random_anc(pos, B, seed=seed + pos)
    scale = 1.0 / math.sqrt(hd)
    return vals, anc, decode_ref(vals, B, H, hd, pos, scale), decode_ref(vals, B, H, hd, pos, scale, anc)


def _padded(vals, pad, dev, fill=NAN):
    """vals in the first columns of a [rows, cols + pad] device buffer filled with `fill`; returns (buffer, view)."""
    buf = torch.full((vals.shape[0], vals.shape[1] + pad), fill, dtype=vals.dtype, device=dev)
    buf[:, : vals.shape[1]] = vals.to(dev)
    return buf, buf[:, : vals.shape[1]]


def _decode(vals, dev, B, H, hd, pos, anc, pad_c, pad_o):
    """One attention_decode launch on `vals` placed in a cache of row stride 3D + pad_c, writing an output of row
    stride D + pad_o. Returns the [B, D] result (CPU) after checking the output's padding columns."""
    D = H * hd
    _, cache = _padded(vals, pad_c, dev)
    obuf = torch.full((B, D + pad_o), SENT, dtype=vals.dtype, device=dev)
    out = obuf[:, :D]
    assert cache.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    ops.attention_decode(cache, out, B=B, H=H, hd=hd, pos=pos, scale=1.0 / math.sqrt(hd),
                         anc=None if anc is None else anc.to(dev))
    assert (obuf[:, D:] == SENT).all(), "decode wrote past its D columns"
    return out.cpu()


def _assert_decode_close(got, ref, absw, dtype):
    got = got.double()
    assert torch.isfinite(got).all(), "decode read a NaN row or padding column"
    err = (got - ref).abs()
    if dtype == F32:
        bound = torch.full_like(ref, 1e-5 * ref.abs().max().item())
    else:
        bound = 2.0 ** -8 * ref.abs() + 1e-4 * absw
    worst = (err / bound).max().item()
    print(f"decode max err/bound = {worst:.3f}, max abs err = {err.max().item():.3e}")
    assert (err <= bound).all(), f"max err/bound {worst:.3f}"


def _decode_case(dev, dtype, B, H, hd, pos, use_anc, pad_c, pad_o, alt_pad=0):
    """alt_pad: the padding of the second layout of check (c); it must keep the launch on the same kernel."""
    D = H * hd
    vals, anc, ref_plain, ref_anc = _decode_data(B, H, hd, pos, dtype)
    if pos:
        assert not torch.equal(anc, identity_anc(pos, B))
    a = anc if use_anc else None
    ref, absw = ref_anc if use_anc else ref_plain
    got = _decode(vals, dev, B, H, hd, pos, a, pad_c, pad_o)
    _assert_decode_close(got, ref, absw, dtype)
    # the arithmetic order depends on n = pos + 1 alone, so these three are bitwise
    if use_anc:  # (b) ancestry == the same rows gathered physically
        gathered = gather_cache(vals, B, D, pos, anc)
        assert torch.equal(got, _decode(gathered, dev, B, H, hd, pos, None, pad_c, pad_o))
    else:        # (a) the identity table == no table
        assert torch.equal(got, _decode(vals, dev, B, H, hd, pos, identity_anc(pos, B), pad_c, pad_o))
    # (c) padded rows == the same data packed
    assert torch.equal(got, _decode(vals, dev, B, H, hd, pos, a, alt_pad, alt_pad))
    return got


@pytest.mark.parametrize("use_anc", [False, True])
@pytest.mark.parametrize("pos", [0, 6, 7, 8, 62, 63, 64, 126, 127, 128, 129, 200])
def test_decode64_bf16(dev, pos, use_anc):
    """attn_decode64_kernel<16>: n = pos + 1 on both sides of one key group (8), one lane pass (64) and the
    register-prefetch depth (128); cache [T*B, 3D + 8] and out [B, D + 8], both used through their packed views."""
    _decode_case(dev, BF16, 3, 3, 64, pos, use_anc, 8, 8)


@pytest.mark.parametrize("use_anc", [False, True])
@pytest.mark.parametrize("pos", [0, 63, 64, 129])
@pytest.mark.parametrize("dtype,hd", [(F32, 32), (F32, 96), (F32, 128), (BF16, 32), (BF16, 96), (BF16, 128),
                                      (BF16, 64)])
def test_decode_generic(dev, dtype, hd, pos, use_anc):
    """attn_decode_kernel<T>: every row stride a multiple of 4 and every base 16-byte aligned (its ld4 loads);
    bf16 hd = 64 reaches it through ld_cache = 3D + 4. For that case the fast kernel on the same data agrees
    within two per-element bounds."""
    B, H = 3, 2
    # bf16 hd = 64 packed (ld = 3D) would be the fast kernel's launch: its second layout keeps ld % 8 == 4
    got = _decode_case(dev, dtype, B, H, hd, pos, use_anc, 4, 4, alt_pad=12 if (dtype == BF16 and hd == 64) else 0)
    if dtype == BF16 and hd == 64:
        vals, anc, ref_plain, ref_anc = _decode_data(B, H, hd, pos, dtype)
        ref, absw = ref_anc if use_anc else ref_plain
        fast = _decode(vals, dev, B, H, hd, pos, anc if use_anc else None, 8, 8)
        diff = (got.double() - fast.double()).abs()
        assert (diff <= 2.0 ** -7 * ref.abs() + 2e-4 * absw).all()


# ------------------------------------------------------------------------------------------ position-major prefill
def _pm(t, B, S):
    """batch-major rows b*S + s -> position-major rows s*B + b"""
    return t.view(B, S, -1).transpose(0, 1).reshape(S * B, -1).contiguous()


def _bm(t, B, S):
    return t.view(S, B, -1).transpose(0, 1).reshape(B * S, -1).contiguous()


def _ref_lse(x, scale, causal, key_mask):
    """fp64 logsumexp of the masked, scaled scores, flattened [B*H*S]; x: [3, B, H, S, hd]"""
    S = x.shape[-2]
    s_ = torch.einsum("bhqd,bhkd->bhqk", x[0], x[1]) * scale
    if causal:
        s_ = s_.masked_fill(torch.ones(S, S, dtype=torch.bool, device=x.device).triu(1), float("-inf"))
    if key_mask is not None:
        s_ = s_.masked_fill(key_mask[:, None, None, :] == 0, float("-inf"))
    return torch.logsumexp(s_, dim=-1).reshape(-1)


PREFILL = ([(BF16, 64, S) for S in (1, 10, 16, 17, 33, 128)] + [(BF16, 64, S) for S in (129, 200)] +
           [(BF16, hd, S) for hd in (96, 128) for S in (10, 50)] + [(F32, 64, S) for S in (10, 65)])


@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("dtype,hd,S", PREFILL)
def test_prefill_position_major(dev, dtype, hd, S, B):
    """attention_fwd(..., causal, rsb=1, rss=B) on rows s*B + b, as GPT2Core's prefill calls it: the fp64
    definition, and bitwise the batch-major launch on the same values (out and lse)."""
    H = 3
    D, scale = H * hd, 1.0 / math.sqrt(hd)
    g = torch.Generator().manual_seed(90 + S + hd)
    qkv_bm = torch.randn((B * S, 3 * D), generator=g).to(dtype).to(dev)
    qkv_pm = _pm(qkv_bm, B, S)
    out_bm, out_pm = (torch.full((B * S, D), SENT, dtype=dtype, device=dev) for _ in range(2))
    lse_bm, lse_pm = (torch.full((B * H * S,), SENT, device=dev) for _ in range(2))
    ops.attention_fwd(qkv_bm, out_bm, B=B, S=S, H=H, hd=hd, scale=scale, causal=True, lse=lse_bm)
    ops.attention_fwd(qkv_pm, out_pm, B=B, S=S, H=H, hd=hd, scale=scale, causal=True, rsb=1, rss=B, lse=lse_pm)
    x = qkv_bm.double().view(B, S, 3, H, hd).permute(2, 0, 3, 1, 4)
    ref = ref_attention(x[0], x[1], x[2], scale, True, None).permute(0, 2, 1, 3).reshape(B * S, D)
    tol = 1e-5 if dtype == F32 else 1e-2
    e = rel_err(_bm(out_pm, B, S), ref)
    print(f"prefill rel_err = {e:.3e}")
    assert e < tol
    assert torch.equal(_bm(out_pm, B, S), out_bm)
    assert torch.equal(lse_pm, lse_bm)
    # lse: 2e-2 is test_attention_long_sequence_forward's bf16 bound; fp32 scores of |s| <~ 8 carry a 64-term dot
    # (64 * 2^-24 * sum|q.k| * scale ~ 2e-5) and one logf
    assert (lse_pm.double() - _ref_lse(x, scale, True, None)).abs().max().item() < (1e-4 if dtype == F32 else 2e-2)


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_prefill_then_decode(dev, dtype):
    """As the engine does it: prefill S = 10 positions of a position-major cache, append position 10's row and
    decode at pos = 10; both match the full causal S = 11 definition."""
    B, H, hd, S = 3, 3, 64, 10
    D, scale = H * hd, 0.125
    g = torch.Generator().manual_seed(95)
    vals = torch.randn(((S + 2) * B, 3 * D), generator=g).to(dtype)
    cache = torch.full(((S + 2) * B, 3 * D), NAN, dtype=dtype, device=dev)
    cache[: S * B] = vals[: S * B].to(dev)
    o = torch.empty((S * B, D), dtype=dtype, device=dev)
    ops.attention_fwd(cache, o, B=B, S=S, H=H, hd=hd, scale=scale, causal=True, rsb=1, rss=B)
    x = vals[: (S + 1) * B].double().view(S + 1, B, 3, H, hd).permute(2, 1, 3, 0, 4)  # [3, B, H, S+1, hd]
    full = ref_attention(x[0], x[1], x[2], scale, True, None)                          # [B, H, S+1, hd]
    ref_pm = full.permute(2, 0, 1, 3).reshape((S + 1) * B, D)
    assert rel_err(o.cpu(), ref_pm[: S * B]) < (1e-5 if dtype == F32 else 1e-2)
    cache[S * B: (S + 1) * B] = vals[S * B: (S + 1) * B].to(dev)
    out = torch.empty((B, D), dtype=dtype, device=dev)
    ops.attention_decode(cache, out, B=B, H=H, hd=hd, pos=S, scale=scale)
    ref, absw = decode_ref(vals, B, H, hd, S, scale)
    assert (ref - ref_pm[S * B:]).abs().max().item() < 1e-12
    _assert_decode_close(out.cpu(), ref, absw, dtype)


# ------------------------------------------------------------------------------------------ fallback MFMA forward
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("hd", [64, 96])
def test_mfma_fallback_forward(dev, hd, causal):
    """amfma::fwd_kernel<64|96>: out = buf[:, 2:2+D] of a [B*S, D + 8] buffer is 4-byte but not 8-byte aligned
    with ld_out % 4 == 0, which the second-generation kernel does not take. Causal runs with a key mask."""
    B, H, S = 2, 3, 50
    D, scale = H * hd, 1.0 / math.sqrt(hd)
    g = torch.Generator().manual_seed(97 + hd)
    qkv = torch.randn((B * S, 3 * D), generator=g).to(BF16).to(dev)
    key_mask = None
    if causal:
        km = torch.ones((B, S), dtype=torch.int32)
        km[0, 30:] = 0
        km[1, 7] = 0
        key_mask = km.to(dev)
    buf = torch.full((B * S, D + 8), SENT, dtype=BF16, device=dev)
    out = buf[:, 2: 2 + D]
    assert out.data_ptr() % 8 == 4 and out.stride(0) % 4 == 0 and qkv.data_ptr() % 16 == 0
    lse = torch.empty(B * H * S, device=dev)
    ops.attention_fwd(qkv, out, B=B, S=S, H=H, hd=hd, scale=scale, causal=causal, key_mask=key_mask, lse=lse)
    x = qkv.double().view(B, S, 3, H, hd).permute(2, 0, 3, 1, 4)
    ref = ref_attention(x[0], x[1], x[2], scale, causal, key_mask).permute(0, 2, 1, 3).reshape(B * S, D)
    e = rel_err(out, ref)
    print(f"fallback rel_err = {e:.3e}")
    assert e < 1e-2
    aligned = torch.empty((B * S, D), dtype=BF16, device=dev)
    lse2 = torch.empty_like(lse)
    ops.attention_fwd(qkv, aligned, B=B, S=S, H=H, hd=hd, scale=scale, causal=causal, key_mask=key_mask, lse=lse2)
    assert rel_err(out, aligned) < 2e-2
    ref_lse = _ref_lse(x, scale, causal, key_mask)
    assert torch.isfinite(ref_lse).all()  # no fully masked row in these cases
    for got_lse in (lse, lse2):  # test_attention_long_sequence_forward's bf16 lse bound
        assert (got_lse.double() - ref_lse).abs().max().item() < 2e-2
    assert (buf[:, :2] == SENT).all() and (buf[:, 2 + D:] == SENT).all()


# ------------------------------------------------------------------------------------------ greedy_next
GREEDY_V = [(50257, 50304), (50, 56), (64, 72), (65, 72)]
FORMS = ["split", "single_no_x", "single_small_d"]


@functools.lru_cache(maxsize=None)
def _greedy_tables(V, D, dtype):
    """(wte [V, D], wpe [10, D]) on the CPU, shared between cases: read-only, callers copy them to the device."""
    g = torch.Generator().manual_seed(61)
    return torch.randn((V, D), generator=g).to(dtype), torch.randn((10, D), generator=g).to(dtype)


def _greedy_case(dev, form, dtype, misaligned, V, ld):
    lg_all, names, winners = special_rows(V, ld, dtype)
    D = 64 if form == "split" else 8
    eos, pos, step = V - 1, 5, 3
    wte, wpe = _greedy_tables(V, D, dtype)
    wted, wped = wte.to(dev), wpe.to(dev)
    R = lg_all.shape[0]
    argmax_checked = set()
    for lo in sorted({0, max(0, R - 8)}):  # launches of B <= 8 rows that together cover every special row
        lg = lg_all[lo: lo + 8]
        B = lg.shape[0]
        if misaligned:  # the same rows one element into a wider buffer: no vector load is aligned (vec 0)
            full = torch.full((B, ld + 8), NAN, dtype=dtype, device=dev)
            lgd = full[:, 1: 1 + ld]
            lgd.copy_(lg)
            assert lgd.data_ptr() % (4 * lgd.element_size()) != 0
        else:
            lgd = lg.to(dev)
            assert lgd.data_ptr() % 16 == 0 and lgd.stride(0) % (8 if dtype == BF16 else 4) == 0
        am = argmax_ref(lg[:, :V])
        assert am.tolist() == winners[lo: lo + 8].tolist()
        # sweep 1: nothing finished, so every row's argmax is asserted; sweeps 2 and 3: one pre-finished row (one
        # whose own argmax is not eos), without and with forced tokens
        k = next(i for i in range(B) if i != 1 and am[i].item() != eos)
        none_fin = torch.zeros(B, dtype=torch.int32)
        one_fin = none_fin.clone()
        one_fin[k] = 1
        forced = (torch.arange(B, dtype=torch.int64) * 5 + 1) % V
        forced[1] = eos
        assert forced[k].item() != eos
        for fin0, f in ((none_fin, None), (one_fin, None), (one_fin, forced)):
            want_tok, want_fin = greedy_bookkeeping(am, fin0, eos, f)
            if f is None and not fin0.any():
                assert want_tok.tolist() == winners[lo: lo + 8].tolist()
                argmax_checked.update(names[lo: lo + 8])
            fd = fin0.to(dev)
            td = torch.full((B, 6), -7, dtype=torch.int64, device=dev)
            xd = None if form == "single_no_x" else torch.full((B, D), SENT, dtype=dtype, device=dev)
            ops.greedy_next(lgd, V, eos, fd, td, step, None if xd is None else wted,
                            None if xd is None else wped, pos, D, xd,
                            forced=None if f is None else f.to(dev))
            t = td.cpu()
            assert t[:, step].tolist() == want_tok.tolist(), (names[lo: lo + 8], fin0.tolist(), f is not None)
            assert (t[:, :step] == -7).all() and (t[:, step + 1:] == -7).all()
            assert fd.cpu().tolist() == want_fin.tolist()
            if fin0.any():
                assert want_fin[k].item() == 1 and want_tok[k].item() == eos
            if xd is not None:
                xr = (wte.float()[want_tok] + wpe.float()[pos]).to(dtype)
                assert torch.equal(xd.cpu(), xr)
    assert argmax_checked == set(names)  # every special row's winner was asserted on an unfinished row


@pytest.mark.parametrize("V,ld", GREEDY_V)
@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("form", FORMS)
def test_greedy_next_forms(dev, form, dtype, misaligned, V, ld):
    """Split (x given, D = 64, V >= 64), single block through x = None, single block through a small D, each with
    16-byte bf16 loads (vec 2), 4-wide fp32 loads (vec 1) and scalar loads from an element-misaligned base
    (vec 0); V = 50 is single block in every form, V = 64 / 65 split with chunk 8 / 16."""
    assert greedy_chunk(64) == 8 and greedy_chunk(65) == 16 and (65 + 15) // 16 == 5
    _greedy_case(dev, form, dtype, misaligned, V, ld)


@pytest.mark.parametrize("form", ["single_no_x", "single_small_d"])
def test_greedy_next_long_row_single_block(dev, form):
    """V = 70001 bf16: rows longer than 8 * 1024 * 8 logits take a second pass of the single block's unrolled loop."""
    _greedy_case(dev, form, BF16, False, 70001, 70008)


# ------------------------------------------------------------------------------------------ glue kernels
def _randn(shape, seed, dtype=F32):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(dtype)


@pytest.mark.parametrize("beam", [False, True])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_add_position(dev, dtype, beam):
    """x[(t*B + b)*D + d] = src[b*sbs + t*sts + d] + wpe[(pos0 + t)*D + d]: one fp32 add, one rounding. beam:
    sbs = 0, one prefix broadcast to every row."""
    B, npos, D, pos0 = 3, 5, 20, 7
    sts = D + 4
    sbs = 0 if beam else npos * sts + 8
    store = _randn((1 if beam else B, npos * sts + 8), 100, dtype)
    src = store[:, : npos * sts].view(-1, npos, sts)[:, :, :D]  # [B or 1, npos, D], strides (sbs or -, sts, 1)
    wpe = _randn((pos0 + npos + 2, D), 101, dtype)
    x = torch.full((npos * B + 1, D), SENT, dtype=dtype, device=dev)
    ops.add_position(store.to(dev), sbs, sts, wpe.to(dev), x, B=B, npos=npos, D=D, pos0=pos0)
    want = (src.float().expand(B, npos, D).transpose(0, 1) + wpe.float()[pos0: pos0 + npos, None, :]).to(dtype)
    assert torch.equal(x[: npos * B].cpu(), want.reshape(npos * B, D))
    assert (x[npos * B:] == SENT).all()


def _embed_want(prefix, wte, wpe, ids, P, L_):
    """fp32 sum before rounding, [B, S, D]"""
    rows = [prefix.float()[:, :P]] if P else []
    if L_:
        rows.append(wte.float()[ids])
    return torch.cat(rows, dim=1) + wpe.float()[None, : P + L_]


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("form", ["padded", "prefix_only", "packed"])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_gpt2_embed(dev, dtype, form, drop):
    """x = (prefix | wte[ids]) + wpe, rounded once; packed sequences write only their live rows at their packed
    rows; dropout keeps exactly the counter-hash mask at index dest_row*D + col and scales by 1/(1-p) in fp32."""
    B, P, L_, D = (3, 10, 0, 24) if form == "prefix_only" else (3, 4, 6, 24)
    S = P + L_
    pbs = P * D if form == "prefix_only" else P * D + 8
    store = _randn((B, pbs), 110, dtype)
    prefix = store[:, : P * D].view(B, P, D)
    wte, wpe = _randn((11, D), 111, dtype), _randn((S + 3, D), 112, dtype)
    ids = None if L_ == 0 else torch.randint(0, 11, (B, L_), generator=torch.Generator().manual_seed(113))
    seqs, lens = None, [S] * B
    if form == "packed":
        lens = [0, 2, S]  # empty, shorter than the prefix, full
        off = [0, 0, 2]
        seqs = (torch.tensor(off, dtype=torch.int32, device=dev), torch.tensor(lens, dtype=torch.int32, device=dev))
    p, seed, offset = 0.25, 0xC0FFEE1234, 11 + (1 << 33)
    x = torch.full((B * S, D), SENT, dtype=dtype, device=dev)
    ops.gpt2_embed(store.to(dev), pbs, wte.to(dev), wpe.to(dev), None if ids is None else ids.to(dev), x,
                   B=B, P=P, L_=L_, D=D, drop=ops.Dropout(p, seed, offset) if drop else ops.NO_DROP, seqs=seqs)
    full = _embed_want(prefix, wte, wpe, ids, P, L_)
    live = torch.cat([full[b, : lens[b]] for b in range(B)], dim=0)  # destination rows in order
    n = live.shape[0]
    assert n == (B * S if seqs is None else 2 + S)
    if drop:
        keep = torch.from_numpy(keep_mask(seed, offset, n * D, p).reshape(n, D))
        inv_keep = torch.tensor(1.0, dtype=F32) / (torch.tensor(1.0, dtype=F32) - torch.tensor(p, dtype=F32))
        assert 0.6 < keep.float().mean().item() < 0.9
        live = torch.where(keep, live * inv_keep, torch.zeros_like(live))
    got = x.cpu()
    assert torch.equal(got[:n], live.to(dtype))
    assert (got[n:] == SENT).all()


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_embedding_scatter_add(dev, dtype):
    """dwte[ids[b, t]] += dx[b*S + P + t] over caption rows only (fp32 atomics, heavy duplicates)."""
    B, P, L_, D, V = 4, 3, 8, 20, 5
    S = P + L_
    dx = _randn((B * S, D), 120, dtype)
    ids = torch.randint(0, V, (B, L_), generator=torch.Generator().manual_seed(121))
    dwte0 = _randn((V, D), 122)
    dwte = dwte0.to(dev)
    ops.embedding_scatter_add(dx.to(dev), ids.to(dev), dwte, B=B, P=P, L_=L_, D=D)
    cap = dx.double().view(B, S, D)[:, P:].reshape(B * L_, D)
    ref = dwte0.double().index_add_(0, ids.reshape(-1), cap)
    mag = dwte0.double().abs().index_add_(0, ids.reshape(-1), cap.abs())
    c = torch.bincount(ids.reshape(-1), minlength=V).double()[:, None]
    assert c.max().item() >= 4  # duplicates
    err = (dwte.cpu().double() - ref).abs()
    assert (err <= (c + 1) * 2.0 ** -24 * mag).all()


@pytest.mark.parametrize("D", [512, 70])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_l2norm_rows(dev, dtype, D):
    R = 5  # not a multiple of the 4 rows a block takes
    xs = _randn((R, D + 6), 130 + D, dtype)
    x = xs.to(dev)[:, :D]
    for rows in (R, 3):
        obuf = torch.full((R, D + 2), SENT, device=dev)
        ops.l2norm_rows(x, obuf[:, :D], rows=rows)
        xd = xs[:rows, :D].double()
        ref = xd / xd.pow(2).sum(dim=1, keepdim=True).sqrt()
        got = obuf.cpu()
        assert (got[:rows, :D].double() - ref).abs().max().item() <= (D + 4) * 2.0 ** -24
        assert (got[rows:] == SENT).all() and (got[:, D:] == SENT).all()


@pytest.mark.parametrize("sdt,ddt", [(F32, BF16), (BF16, F32), (F32, F32), (BF16, BF16)])
def test_convert(dev, sdt, ddt):
    M, N = 7, 13
    src = _randn((M, N + 3), 140, sdt)
    if sdt == F32:  # round-to-nearest-even ties both ways, signed zeros, infinities, overflow to inf, NaN
        bits = np.array([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF], dtype=np.uint32)
        src[0, :6] = torch.from_numpy(bits.view(np.float32))
        src[1, :7] = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), 3.4e38, -3.4e38, NAN])
    dbuf = torch.full((M, N + 5), SENT, dtype=ddt, device=dev)
    ops.convert(src.to(dev)[:, :N], dbuf[:, :N])
    got, want = dbuf.cpu()[:, :N], src[:, :N].to(ddt)
    nan = want.isnan()
    assert torch.equal(got.isnan(), nan)
    assert torch.equal(got[~nan], want[~nan])
    assert torch.equal(torch.signbit(got[~nan]), torch.signbit(want[~nan]))  # -0 stays -0
    if sdt == F32 and ddt == BF16:
        assert got[0, :4].float().tolist() == [1.0, 1.015625, -1.0, -1.015625]
        assert got[1, 4].item() == float("inf") and got[1, 5].item() == float("-inf")
    assert (dbuf[:, N:] == SENT).all()


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_broadcast_rows(dev, dtype):
    R, D, B = 3, 20, 4
    bs = R * D + 12
    src = _randn((R, D), 150)
    dst = torch.full((B * bs,), SENT, dtype=dtype, device=dev)
    ops.broadcast_rows(src.to(dev), dst, B, bs)
    got = dst.cpu().view(B, bs)
    assert torch.equal(got[:, : R * D], src.to(dtype).reshape(1, R * D).expand(B, R * D))
    assert (got[:, R * D:] == SENT).all()


@pytest.mark.parametrize("n", [1, 255, 100003])
def test_sqnorm(dev, n):
    x = _randn((n,), 160 + n)
    out = torch.full((1,), SENT, device=dev)
    ws = torch.empty(ops.adamw_workspace(n) // 4, device=dev)
    ops.sqnorm(x.to(dev), out, ws)
    ref = x.double().pow(2).sum().item()
    assert abs(out.item() - ref) / ref < 1e-6
