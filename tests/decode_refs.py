"""Plain torch fp64 restatements (CPU tensors) of what the decode-time kernels compute, and the shared inputs of
their tests: test_decode_refs_cpu.py checks these references against independent definitions without a GPU,
test_decode_kernels_gpu.py checks the kernels against them.
"""

import functools

import torch

GSPLIT = 8  # csrc/elementwise.hip: column ranges per row of the split greedy_next


def decode_ref(cache, B, H, hd, pos, scale, anc=None):
    """Decode attention of the query at position `pos` over keys 0..pos of a position-major cache.

    cache: rows t*B + b, columns [q | k | v] (3*H*hd wide; wider rows are ignored past that). The query is row
    (pos, b); key / value j comes from row (j, anc[j, b]) when anc (int [>= pos+1, B]) is given, else (j, b).
    Returns (out, absw), both fp64 [B, H*hd]: out = sum_j p_j v_j with p = softmax_j(scale * q.k_j) and
    absw = sum_j p_j |v_j|, the magnitude an accumulation-error bound scales with."""
    D = H * hd
    n = pos + 1
    c = cache.detach().cpu()[: n * B, : 3 * D].double().reshape(n, B, 3, H, hd)
    q = c[pos, :, 0]                  # [B, H, hd]
    k, v = c[:, :, 1], c[:, :, 2]     # [n, B, H, hd]
    if anc is not None:
        idx = anc.detach().cpu()[:n].long().reshape(n, B, 1, 1).expand(n, B, H, hd)
        k, v = torch.gather(k, 1, idx), torch.gather(v, 1, idx)
    s = torch.einsum("bhd,jbhd->bhj", q, k) * scale
    p = torch.softmax(s, dim=-1)
    out = torch.einsum("bhj,jbhd->bhd", p, v)
    absw = torch.einsum("bhj,jbhd->bhd", p, v.abs())
    return out.reshape(B, D), absw.reshape(B, D)


def gather_cache(cache, B, D, pos, anc):
    """A copy of `cache` whose k / v columns at row (j, b), j <= pos, are those of row (j, anc[j, b]); q columns
    and everything else unchanged. decode(cache, anc) reads exactly what decode(gather_cache(...), None) reads."""
    n = pos + 1
    out = cache.clone()
    a = anc.detach().to(cache.device)[:n].long()                               # [n, B]
    rows = (torch.arange(n, device=cache.device)[:, None] * B + a).reshape(-1)  # source row of (j, b)
    out[: n * B, D: 3 * D] = cache[rows, D: 3 * D]
    return out


def random_anc(pos, B, seed):
    """int32 [pos+1, B] ancestry, uniform in [0, B), with anc[pos, b] = b (beam search writes row pos itself)."""
    g = torch.Generator().manual_seed(seed)
    anc = torch.randint(0, B, (pos + 1, B), generator=g, dtype=torch.int32)
    anc[pos] = torch.arange(B, dtype=torch.int32)
    return anc


def identity_anc(pos, B):
    return torch.arange(B, dtype=torch.int32).repeat(pos + 1, 1)


def argmax_ref(logits):
    """torch.argmax over the last dimension of the float view: the first NaN wins, ties go to the smallest index
    (an all -inf row gives 0). Pass logits[:, :V]."""
    return torch.argmax(logits.detach().cpu().float(), dim=-1)


def greedy_bookkeeping(argmax_tok, finished, eos, forced=None):
    """Host restatement of greedy_next's per-row bookkeeping: a forced token overrides the argmax, a finished row
    emits eos, and emitting eos latches finished. Returns (tokens int64 [B], finished int32 [B])."""
    tok = (argmax_tok if forced is None else forced).clone().long()
    fin = finished.bool()
    tok[fin] = eos
    fin = fin | (tok == eos)
    return tok, fin.to(torch.int32)


def greedy_chunk(V):
    """Columns per block of the split greedy_next (csrc/elementwise.hip icap_greedy_next)."""
    return ((V + GSPLIT - 1) // GSPLIT + 7) // 8 * 8


HI = 50.0  # a planted winner: far above every N(0,1) background logit, exact in bf16


def special_rows(V, ld, dtype, seed=70):
    """Logits [R, ld] of `dtype` (CPU) with one hand-made case per row, the name of each row and the winner written
    down by hand. Background N(0,1); columns [V, ld) of every row hold +inf and NaN (never to be read). Rows whose
    indices do not exist at this V are left out. Built once per (V, ld, dtype); every call gets its own copies."""
    lg, names, winners = _special_rows(V, ld, dtype, seed)
    return lg.clone(), list(names), winners.clone()


@functools.lru_cache(maxsize=None)
def _special_rows(V, ld, dtype, seed):
    chunk = greedy_chunk(V)
    v8 = V & ~7
    nan, inf = float("nan"), float("inf")
    cases = [
        ("first", {0: HI}, 0),
        ("last", {V - 1: HI}, V - 1),
        ("vector_end", {v8 - 1: HI}, v8 - 1),
        ("scalar_tail", {v8: HI}, v8),
        ("chunk_end", {chunk - 1: HI}, chunk - 1),
        ("chunk_start", {chunk: HI}, chunk),
        ("tie_chunk_edge", {chunk - 1: HI, chunk: HI}, chunk - 1),
        ("tie_far", {5: HI, 3 * chunk + 1: HI}, 5),
        ("two_nans", {chunk + 3: nan, 3 * chunk + 1: nan, 2 * chunk + 2: HI}, chunk + 3),
        ("plus_inf", {3: HI, V // 2: inf}, V // 2),
        ("all_minus_inf", None, 0),
        ("padding", {17: HI}, 17),
    ]
    g = torch.Generator().manual_seed(seed)
    rows, names, winners = [], [], []
    for name, plant, win in cases:
        if plant is not None and not all(0 <= j < V for j in plant):
            continue
        r = torch.randn(ld, generator=g)
        if plant is None:
            r[:V] = -inf
        else:
            for j, val in plant.items():
                r[j] = val
        r[V::2] = inf
        r[V + 1::2] = nan
        rows.append(r)
        names.append(name)
        winners.append(win)
    return torch.stack(rows).to(dtype), names, torch.tensor(winners, dtype=torch.int64)
