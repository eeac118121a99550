"""fp64 references (CPU tensors) of every dropout site, built from the restated counter-based mask
(test_dropout_hash.keep_mask, include/icap.h "Dropout"), and the shared inputs of their tests:
test_dropout_refs_cpu.py checks the references on their own without a GPU, test_dropout_sites_gpu.py checks the
kernels against them and test_dropout_step_gpu.py the whole train step against the oracle run under MaskedOracle.

The mask is a pure function of (seed, device counter, offset, element index), so a reference can use exactly the
masks the device draws. The descriptor's p reaches the device as a float (icap_*_args.drop_p): threshold and scale
are taken from that float here too (host_common.h drop_threshold, 1.f / (1.f - p)).
"""

import functools
import math

import numpy as np
import torch

from oracle import icap_oracle as O
from test_dropout_hash import eff_seed, hash32, keep_mask, threshold

BIG_SEED = 0xDEADBEEF12345678   # bits above 32 set
BIG_OFFSET = 5 + (1 << 40)      # the mapper's base (TransformerMapperCore.drops) + 5
CTR_SEED, CTR_OFFSET, CTR_VALUE = 99, 7, 3


class Desc:
    """What site_keep / attn_keep read of an ops.Dropout: p, seed, offset, counter (tensor or None)."""

    def __init__(self, p, seed, offset, counter=None):
        self.p, self.seed, self.offset, self.counter = float(p), int(seed) & (2 ** 64 - 1), int(offset), counter

    def at(self, offset):
        return Desc(self.p, self.seed, offset, self.counter)


def p32(p):
    return float(np.float32(p))


def inv_keep(p):
    return 1.0 / (1.0 - p32(p))


def _counter(drop, counter):
    if counter is None and drop.counter is not None:
        counter = int(drop.counter)
    return counter


def site_keep(drop, shape, counter=None, rows=None):
    """bool keep tensor of `shape` for descriptor `drop` over a row-major tensor: element (r, c) of the [R, D]
    flattening (D = shape[-1]) has index offset + r*D + c. counter: the device counter's value (None: read from
    drop.counter when it has one). rows: int array [R], the device row of logical row r (packed layouts); a
    negative entry is a row the device never computes and keeps everything."""
    shape = tuple(shape)
    n, D = int(np.prod(shape)), shape[-1]
    counter = _counter(drop, counter)
    if rows is None:
        k = keep_mask(drop.seed, drop.offset, n, p32(drop.p), counter)
    else:
        rows = np.asarray(rows, dtype=np.int64)
        assert rows.shape == (n // D,)
        idx = np.maximum(rows, 0)[:, None] * D + np.arange(D, dtype=np.int64)[None, :]
        h = hash32(eff_seed(drop.seed, counter), np.uint64(drop.offset) + idx.astype(np.uint64))
        k = h >= np.uint32(threshold(p32(drop.p)))
        k[rows < 0] = True
    return torch.from_numpy(np.ascontiguousarray(k.reshape(shape)))


def attn_keep(drop, B, H, S, counter=None):
    """bool [B, H, S, S]: index offset + (b*H + h)*S*S + q*S + k (include/icap.h icap_attn_args)."""
    return site_keep(drop, (B, H, S, S), counter)


def packed_rows(seq_off, seq_len, S):
    """rows argument of site_keep for a [B, S, D] site of the packed step: position (b, t) is device row
    seq_off[b] + t for t < seq_len[b]; later positions are never computed (-1)."""
    rows = np.full((len(seq_len), S), -1, np.int64)
    for b, (o, n) in enumerate(zip(seq_off, seq_len)):
        rows[b, :n] = o + np.arange(n)
    return rows.reshape(-1)


def allowed_mask(B, S, causal, key_mask):
    a = torch.ones((S, S), dtype=torch.bool)
    if causal:
        a = torch.tril(a)
    a = a[None, None].expand(B, 1, S, S)
    if key_mask is not None:
        a = a & key_mask.bool().reshape(B, 1, 1, S)
    return a


def ref_attention_drop(q, k, v, scale, causal, key_mask, keep, p):
    """q, k, v: fp64 [B, H, S, hd]; keep: bool [B, H, S, S] or None. Returns (out [B, H, S, hd], lse [B, H, S]):
    out = (softmax(s) * keep / (1 - p)) @ v with s = scale * q k^T under the mask rule of icap_attn_args, lse the
    logsumexp of s without dropout. A query row with no allowed key gives out = 0 (and a zero gradient) and
    lse = -inf."""
    B, _, S, _ = q.shape
    allowed = allowed_mask(B, S, causal, key_mask)
    s = (q @ k.transpose(-1, -2)) * scale
    s = s.masked_fill(~allowed, float("-inf"))
    live = allowed.any(-1, keepdim=True)
    pr = torch.softmax(torch.where(live, s, torch.zeros_like(s)), -1) * live
    with torch.no_grad():
        lse = torch.logsumexp(s, -1)
    if keep is not None:
        pr = pr * keep * inv_keep(p)
    return pr @ v, lse


# ------------------------------------------------------------------------------------------------ descriptors


def make_desc(p, big):
    """(Desc with no counter tensor, counter value): the two ways every family is checked — a seed with bits above
    32 set at offset 5 + 2^40 without a counter, or a small seed / offset with a device counter holding 3."""
    return (Desc(p, BIG_SEED, BIG_OFFSET), None) if big else (Desc(p, CTR_SEED, CTR_OFFSET), CTR_VALUE)


def variants(d, counter, shape, attn=False, ld=None):
    """The wrong masks a reference must tell from the right one: the offset shifted by one, and the two indices
    swapped (q*S+k -> k*S+q for attention; for an [M, N] site the column-major index, and with ld the row stride
    ld in place of N)."""
    out = {"offset+1": site_keep(d.at(d.offset + 1), shape, counter)}
    if attn:
        out["swapped"] = site_keep(d, shape, counter).transpose(-1, -2).contiguous()
    else:
        M, N = shape
        out["swapped"] = site_keep(d, (N, M), counter).t().contiguous()
        if ld is not None:
            out["ld"] = site_keep(d, (M, ld), counter)[:, :N].contiguous()
    return out


# ------------------------------------------------------------------------------------------------ attention


def randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


class AttnCase:
    def __init__(self, name, dtype, S, hd, causal, masked, p=0.1, big=False, bwd=True, B=2, H=2, hide0=False):
        self.name, self.dtype, self.B, self.S, self.H, self.hd = name, dtype, B, S, H, hd
        self.causal, self.masked, self.p, self.big, self.bwd, self.hide0 = causal, masked, p, big, bwd, hide0
        self.scale = 1.0 / math.sqrt(hd)

    def __repr__(self):
        return self.name

    def key_mask(self):
        """int32 [B, S] or None. masked: a ragged tail (batch row 0 loses its last 3 keys, row 1 its second half);
        hide0: key 0 of batch row 1 hidden, so under causal its query 0 has no allowed key."""
        if not (self.masked or self.hide0):
            return None
        km = torch.ones((self.B, self.S), dtype=torch.int32)
        if self.masked:
            km[0, self.S - 3:] = 0
            km[1, self.S // 2:] = 0
        if self.hide0:
            km[1, 0] = 0
        return km

    def inputs(self):
        """(qkv [B*S, 3D], dout [B*S, D]) in the case's dtype (CPU)."""
        D = self.H * self.hd
        return (randn((self.B * self.S, 3 * D), 20 + self.S).to(self.dtype),
                randn((self.B * self.S, D), 21 + self.S).to(self.dtype))

    def desc(self):
        return make_desc(self.p, self.big)


bf, f32 = torch.bfloat16, torch.float32
# kernel reached (csrc/attention_mfma.hip mfma_attention_launch, csrc/attention.hip): bf16 hd 64 / 96 / 128 at
# S <= 128 -> fwd2_kernel<hd>; backward with O -> bwd2_kernel<hd>, without -> bwd_kernel<64 / 96> (hd 128: the VALU
# attn_bwd_kernel<bf16>); bf16 hd 64 / 96 at S > 128 -> fwd3_kernel<hd> (forward only); fp32 and bf16 hd 16 -> the
# VALU attn_fwd_kernel / attn_bwd_kernel.
ATTN_CASES = [
    AttnCase("v2-64-S16", bf, 16, 64, True, True, big=True),
    AttnCase("v2-64-S33", bf, 33, 64, True, True),
    AttnCase("v2-64-S65-p.5", bf, 65, 64, True, True, p=0.5, big=True),
    AttnCase("v2-64-S128", bf, 128, 64, True, True),
    AttnCase("v2-96-S25", bf, 25, 96, False, False, big=True),
    AttnCase("v2-128-S25", bf, 25, 128, True, True),
    AttnCase("v2-128-S60", bf, 60, 128, True, True, big=True),
    AttnCase("v3-64-S129", bf, 129, 64, True, True, bwd=False),
    AttnCase("v3-64-S257", bf, 257, 64, True, True, big=True, bwd=False),
    AttnCase("v3-96-S129-p.5", bf, 129, 96, True, True, p=0.5, bwd=False),
    AttnCase("valu-f32-S65", f32, 65, 64, True, True, big=True),
    AttnCase("valu-bf16-hd16-S9", bf, 9, 16, False, False),
]
# query 0 of batch row 1 has no allowed key (causal, key 0 hidden)
HIDE0_CASES = [
    AttnCase("hide0-v2-64-S33", bf, 33, 64, True, False, hide0=True),
    AttnCase("hide0-v3-64-S129", bf, 129, 64, True, False, hide0=True, big=True, bwd=False),
    AttnCase("hide0-valu-f32-S33", f32, 33, 64, True, False, hide0=True, big=True),
    AttnCase("hide0-valu-bf16-hd16-S9", bf, 9, 16, True, False, hide0=True),
]


def attn_tols(dtype):
    """(out, dqkv, lse) bounds: test_kernels_gpu.py test_attention / test_attention_long_sequence_forward — max-abs
    over max-ref for out and dqkv, max-abs for lse."""
    return (1e-5, 1e-5, 1e-5) if dtype == torch.float32 else (1e-2, 2e-2, 2e-2)


def attn_reference(qkv, dout, B, S, H, hd, scale, causal, key_mask, keep, p):
    """(out [B*S, D], lse [B*H*S], dqkv [B*S, 3D] or None) in fp64 from the token-major fused qkv the kernels read."""
    D = H * hd
    x = qkv.double().view(B, S, 3, H, hd).permute(2, 0, 3, 1, 4).detach().requires_grad_(dout is not None)
    o, lse = ref_attention_drop(x[0], x[1], x[2], scale, causal, key_mask, keep, p)
    o2 = o.permute(0, 2, 1, 3).reshape(B * S, D)
    g = None
    if dout is not None:
        (gx,) = torch.autograd.grad(o2, x, dout.double())
        g = gx.permute(1, 3, 0, 2, 4).reshape(B * S, 3 * D)
    return o2.detach(), lse.reshape(-1), g


@functools.lru_cache(maxsize=None)
def attn_case_reference(case, variant=None):
    """The reference of an AttnCase (variant: None, or a key of variants() — a deliberately wrong mask)."""
    qkv, dout = case.inputs()
    d, ctr = case.desc()
    shape = (case.B, case.H, case.S, case.S)
    keep = attn_keep(d, case.B, case.H, case.S, ctr) if variant is None else variants(d, ctr, shape, True)[variant]
    return attn_reference(qkv, dout if case.bwd else None, case.B, case.S, case.H, case.hd, case.scale, case.causal,
                          case.key_mask(), keep, case.p)


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


# ------------------------------------------------------------------------------------------------ GEMM epilogue


class GemmCase:
    def __init__(self, name, dtype, M, N, K, p=0.1, big=False, split_k=0, ldc=None):
        self.name, self.dtype, self.M, self.N, self.K = name, dtype, M, N, K
        self.p, self.big, self.split_k, self.ldc = p, big, split_k, ldc

    def __repr__(self):
        return self.name

    def inputs(self):
        """A [M, K], B [N, K], bias [N] (fp32), resid [M, N], and the backward's G [M, Kb], W [N, Kb] (CPU); Kb = 64,
        or K where the case forces a split of K."""
        M, N, K, dt = self.M, self.N, self.K, self.dtype
        Kb = K if self.split_k > 1 else 64
        return dict(A=randn((M, K), 6, 0.1).to(dt), B=randn((N, K), 7, 0.1).to(dt), bias=randn((N,), 8, 0.5),
                    resid=randn((M, N), 9).to(dt), G=randn((M, Kb), 10, 8.0 / math.sqrt(Kb)).to(dt),
                    W=randn((N, Kb), 11).to(dt))

    def desc(self):
        return make_desc(self.p, self.big)


BWD_ALPHA = 0.5
GEMM_CASES = [
    GemmCase("edge-bf16", bf, 130, 200, 72, big=True),
    GemmCase("edge-f32", f32, 130, 200, 72),
    GemmCase("skinny-bf16-p.5", bf, 7, 768, 256, p=0.5),
    GemmCase("skinny-f32", f32, 7, 768, 256, big=True),
    GemmCase("splitk3-bf16", bf, 128, 768, 1024, split_k=3),
    GemmCase("ldc208-bf16", bf, 130, 200, 72, ldc=208),
    GemmCase("ldc208-f32", f32, 130, 200, 72, big=True, ldc=208),
]


def gemm_tol(dtype):
    return 1e-5 if dtype == torch.float32 else 1e-2  # test_kernels_gpu.py test_gemm_epilogues


def gemm_reference(case, keep, aux=None):
    """fp64: z = A B^T + bias; resid form C = keep*z/(1-p) + resid (GPT-2 ra / rm); relu form aux = z,
    C = keep*relu(z)/(1-p) (the mapper's dff); backward dZ = alpha*(G W^T)*keep/(1-p)*[aux > 0] with `aux` the
    tensor the backward reads (None: the reference's own z)."""
    t = {k: v.double() for k, v in case.inputs().items()}
    s = inv_keep(case.p)
    z = t["A"] @ t["B"].t() + t["bias"]
    src = z if aux is None else aux.detach().double().cpu()
    return dict(z=z, resid=keep * z * s + t["resid"], relu=keep * torch.relu(z) * s,
                dz=BWD_ALPHA * (t["G"] @ t["W"].t()) * keep * s * (src > 0))


@functools.lru_cache(maxsize=None)
def gemm_keep(case, variant=None):
    d, ctr = case.desc()
    if variant is None:
        return site_keep(d, (case.M, case.N), ctr)
    return variants(d, ctr, (case.M, case.N), ld=case.ldc)[variant]


# ------------------------------------------------------------------------------------------------ layernorm_bwd


class LnCase:
    def __init__(self, name, dtype, rows, D, p=0.1, big=False, dres=False, params=True, rows_dev=None, rowmap=False):
        self.name, self.dtype, self.rows, self.D, self.p, self.big = name, dtype, rows, D, p, big
        self.dres, self.params, self.rows_dev, self.rowmap = dres, params, rows_dev, rowmap

    def __repr__(self):
        return self.name

    def inputs(self):
        """x, dy, dres [rows, D]; gamma, beta [D] (fp32); rowmap int32 [rows] or None: a permutation of the dy rows
        with every fourth entry negative (that row's dy is zero)."""
        rows, D, dt = self.rows, self.D, self.dtype
        rm = None
        if self.rowmap:
            rm = torch.randperm(rows, generator=torch.Generator().manual_seed(17)).to(torch.int32)
            rm[::4] = -1
        return dict(x=(randn((rows, D), 12, 2.0) + 0.5).to(dt), gamma=randn((D,), 13) * 0.2 + 1,
                    beta=randn((D,), 14) * 0.1, dy=randn((rows, D), 15).to(dt),
                    dres=randn((rows, D), 16).to(dt) if self.dres else None, rowmap=rm)

    def desc(self):
        return make_desc(self.p, self.big)


# (rows, D): 768 / 1024 / 1280 / 1536 reach ln_bwd8_kernel's 3 / 4 / 5 / 6 column groups, 132 (not a multiple of 8)
# the 4-wide ln_bwd_kernel (csrc/layernorm.hip icap_layernorm_bwd)
LN_SHAPES = [(37, 768), (9, 1024), (9, 1280), (9, 1536), (9, 132)]
LN_CASES = [LnCase(f"{r}x{D}-{'bf16' if dt == bf else 'f32'}", dt, r, D, big=(i + j) % 2 == 0)
            for i, (r, D) in enumerate(LN_SHAPES) for j, dt in enumerate((bf, f32))]
LN_CASES += [
    LnCase("dres-37x768-bf16-p.5", bf, 37, 768, p=0.5, dres=True),
    LnCase("noparams-37x768-f32", f32, 37, 768, big=True, dres=True, params=False),
    LnCase("rowsdev29-37x768-bf16", bf, 37, 768, big=True, rows_dev=29),
    LnCase("rowmap-9x132-f32", f32, 9, 132, rowmap=True),
]


def ln_tols(dtype):
    """(dx and dx_drop, dgamma, dbeta): test_kernels_gpu.py test_layernorm."""
    return (1e-5, 1e-5, 1e-5) if dtype == torch.float32 else (2e-2, 1e-2, 1e-5)


def ln_reference(case, keep, eps=1e-5):
    """fp64 (dx, dx_drop, dgamma, dbeta) over the first rows_dev rows (all when None):
    dx = LN'(x)^T dy (+ dres), dx_drop = dx * keep / (1 - p)."""
    t = case.inputs()
    n = case.rows if case.rows_dev is None else case.rows_dev
    x = t["x"].double()[:n].requires_grad_(True)
    g = t["gamma"].double().requires_grad_(True)
    b = t["beta"].double().requires_grad_(True)
    dy = t["dy"].double()
    if t["rowmap"] is not None:
        rm = t["rowmap"].long()
        dy = torch.where((rm >= 0)[:, None], dy[rm.clamp_min(0)], torch.zeros_like(dy))
    y = torch.nn.functional.layer_norm(x, (case.D,), g, b, eps)
    gx, gg, gb = torch.autograd.grad(y, (x, g, b), dy[:n])
    if t["dres"] is not None:
        gx = gx + t["dres"].double()[:n]
    return gx, gx * keep[:n] * inv_keep(case.p), gg, gb


@functools.lru_cache(maxsize=None)
def ln_keep(case, variant=None):
    d, ctr = case.desc()
    if variant is None:
        return site_keep(d, (case.rows, case.D), ctr)
    return variants(d, ctr, (case.rows, case.D), ld=case.D + 8)[variant]


# ------------------------------------------------------------------------------------------------ whole step


class MaskedOracle:
    """Context manager: while active, oracle.icap_oracle._drop multiplies by the masks trainer `t` draws in its
    next / last step, x * keep / (1 - p), instead of drawing from torch's generator.

    One `with` block is one train-mode evaluation (mapper_forward then caption_forward). The sites are consumed in
    the oracle's call order — the mapper, per layer: attn, d1, dff, d2; then GPT-2: embd, then per layer attn, ra,
    rm — from the trainer's own descriptors t.mdr / t.gdr (TransformerMapperCore.drops / GPT2Core.drops), with the
    counter value int(t.counter) read on entry (the value the step that just ran used). Leaving the block asserts
    the list is exactly exhausted. A call with train false (or p == 0) passes through and consumes nothing (a
    whole evaluation with train false leaves the list untouched, which is accepted).
    grows: site_keep's rows for the GPT-2 [B, S, D] sites (packed_rows(...) for the packed step; attention keeps
    the padded numbering either way)."""

    def __init__(self, t, mapper_layers, gpt_layers, grows=None):
        self.t, self.ml, self.gl, self.grows = t, mapper_layers, gpt_layers, grows
        self.sites, self.calls = [], 0

    def _sites(self):
        m, g = self.t.mdr, self.t.gdr
        s = []
        for l in range(self.ml):
            s += [("attn", m.attn(l), None), ("rows", m.d1(l), None), ("rows", m.dff(l), None),
                  ("rows", m.d2(l), None)]
        s.append(("rows", g.embd, self.grows))
        for l in range(self.gl):
            s += [("attn", g.attn(l), None), ("rows", g.ra(l), self.grows), ("rows", g.rm(l), self.grows)]
        return s

    def _hook(self, x, p, train):
        if not (train and p > 0):
            return x
        assert self.sites, "more dropout calls than the step has sites"
        kind, d, rows = self.sites.pop(0)
        self.calls += 1
        assert abs(d.p - p) < 1e-6, (kind, d.p, p)
        if kind == "attn":
            assert x.dim() == 4 and x.shape[-1] == x.shape[-2], x.shape
        keep = site_keep(d, x.shape, self.counter, rows)
        return x * keep * inv_keep(d.p)

    def __enter__(self):
        self.counter = int(self.t.counter)
        self.sites, self.calls = self._sites(), 0
        self._saved = O._drop
        O._drop = self._hook
        return self

    def __exit__(self, et, ev, tb):
        O._drop = self._saved
        if et is None and self.calls:  # (an evaluation with train false consumes nothing)
            assert not self.sites, f"{len(self.sites)} dropout sites left unconsumed"
        return False
