"""The epilogue operands issued under the main loop (round 8): the split-role ring kernels on 96 x 128 and 160 x 128
tiles (csrc/gemm_tile.h ROLES / HOIST, variants 27 / 32 = roles 96 / 160) load the bias / ln_wsum columns, the dropout
seed's device counter and the first prefetch group of residual / dact_src rows in front of the K loop, and sum the
statistics producer's quads by DPP. Nothing about the arithmetic changes, so every output is bitwise what the 128-row
tile path (tile_only=True, split_k=1: kernels the change does not touch) gives. The 128 x 256 tiles (roles 256: no
registers for it) and the 8-phase kernel (csrc/gemm8p.hip: measured, no gain) keep their loads after the loop
(DESIGN.md, round 8); the same cases run on them, so a later hoist there meets the same checks.

What could go wrong and where it would show: an operand loaded for the wrong tile, row or column (blocks that walk
several tiles, partial row / column tiles, a device row count that ends inside a tile or is 0), a load that is used
before it landed or that disturbs the ring's counted DMA waits (K from one k-step to one more than the ring's depth,
K tails), and the forms that keep the old path (partial-width lanes at N = 130, fp32 C)."""

import pytest
import torch

from icap import _lib as L
from icap import ops
from gemm_helpers import _assert_same, _run, rnd

pytestmark = pytest.mark.gpu

# variant -> (BM, BN, ring stages, ops.gemm keywords); the 8-phase kernel has no ring depth of its own (K-tiles of 64)
GEO = {96: (96, 128, 5, dict(roles=96)), 160: (160, 128, 4, dict(roles=160)), 256: (128, 256, 3, dict(roles=256)),
       "g8p": (256, 256, 3, dict(g8p=256))}
CONSUMERS = (256, "g8p")  # the variants with the LayerNorm-fold consumer
FILL = -7.0


def _ks(variant):
    nst = GEO[variant][2]
    return sorted({64, 128, (nst - 1) * 64, nst * 64, (nst + 1) * 64, 200})


def _is_native(variant, name):
    return "gemm8p_kernel" in name if variant == "g8p" else (name.endswith(", true>") and "gemm_kernel" in name)


def _padded(shape, dev, ld, dtype=torch.bfloat16, seed=0, fill=None):
    """An [M, N] view of an [M, ld] buffer (ld % 8 == 0: the 16-byte prefetch path also at N = 130)."""
    M, N = shape
    buf = torch.full((M, ld), fill, device=dev, dtype=dtype) if fill is not None else rnd((M, ld), dev, dtype, seed=seed)
    return buf[:, :N]


class _Case:
    """Seeded operands of one (M, N, K); launch(form, kw) runs one epilogue form and returns its named outputs."""

    def __init__(self, dev, M, N, K, c_dtype=torch.bfloat16, m_dev=None, counter=None):
        self.dev, self.M, self.N, self.K, self.c_dtype = dev, M, N, K, c_dtype
        self.ld = (N + 7) // 8 * 8
        self.A = rnd((M, K), dev, scale=0.5, seed=1)
        self.B = rnd((N, K), dev, scale=0.1, seed=2)
        self.bias = rnd((N,), dev, torch.float32, 0.5, seed=3)
        self.resid = _padded((M, N), dev, self.ld, seed=4)
        self.dsrc = _padded((M, N), dev, self.ld, seed=5)
        self.wsum = rnd((N,), dev, torch.float32, 0.3, seed=6)
        self.drop = ops.Dropout(0.1, seed=1234, offset=77, counter=counter)
        self.md = {} if m_dev is None else dict(m_dev=torch.tensor([m_dev], dtype=torch.int32, device=dev), m_hint=m_dev)
        if K % 32 == 0:  # the producer's hand-off for the consumer forms: (mean, M2) per row and 32-column group of A
            grp = self.A.float().view(M, K // 32, 32)
            mean = grp.mean(-1)
            self.stats = torch.stack((mean, ((grp - mean[..., None]) ** 2).sum(-1)), -1).contiguous()

    def out(self):
        return _padded((self.M, self.N), self.dev, self.ld, self.c_dtype, fill=FILL)

    def launch(self, form, kw):
        A, B, C = self.A, self.B, self.out()
        kw = dict(kw, split_k=1, **self.md)
        res = [("C", C)]
        if form == "bias":
            ops.gemm(A, B, C, bias=self.bias, **kw)
        elif form == "rd":
            ops.gemm(A, B, C, bias=self.bias, resid=self.resid, drop=self.drop, alpha=0.75, **kw)
        elif form == "rd_lns":
            st = torch.full((self.M, self.N // 32, 2), FILL, device=self.dev)
            ops.gemm(A, B, C, bias=self.bias, resid=self.resid, drop=self.drop, alpha=0.75, ln_stats_out=st, **kw)
            res.append(("stats", st.view(self.M, -1)))
        elif form in ("lnf", "lnf_gelu"):
            mo, ro = torch.full((self.M,), FILL, device=self.dev), torch.full((self.M,), FILL, device=self.dev)
            extra = {}
            if form == "lnf_gelu":
                aux = self.out()
                extra = dict(act=L.ACT_GELU_NEW, aux=aux)
                res.append(("aux", aux))
            ops.gemm(A, B, C, bias=self.bias, ln_fold=(self.wsum, 1e-5), ln_stats_in=self.stats, ln_rows_out=(mo, ro),
                     **extra, **kw)
            res += [("mean", mo[:, None]), ("rstd", ro[:, None])]
        elif form == "dgelu":
            ops.gemm(A, B, C, dact=L.ACT_GELU_NEW, dact_src=self.dsrc, drop=self.drop, alpha=0.5, **kw)
        else:
            raise ValueError(form)
        return res


def _forms(variant, N, K):
    forms = ["bias", "rd", "dgelu"]
    if N % 32 == 0:
        forms.append("rd_lns")
    if variant in CONSUMERS and K % 128 == 0:
        forms += ["lnf", "lnf_gelu"]
    return forms


def _compare(variant, case, forms, untouched=False):
    """Every form on the changed kernel and on the tile path: the right kernel ran, all outputs bitwise equal
    (unwritten rows and padding keep the fill on both sides); untouched: nothing at all was written."""
    kw = GEO[variant][3]
    for form in forms:
        got, ref = {}, {}
        names = _run(lambda: got.update(case.launch(form, kw)))
        assert len(names) == 1 and _is_native(variant, names[0]), (form, names)
        tnames = _run(lambda: ref.update(case.launch(form, dict(tile_only=True))))
        assert not any(_is_native(variant, n) for n in tnames), (form, tnames)
        torch.cuda.synchronize()
        for name in ref:
            _assert_same(f"{form} {name}", got[name], ref[name])
            if untouched:
                assert bool((got[name] == FILL).all()), (form, name)


VARIANT_K = [(v, K) for v in GEO for K in _ks(v)]


@pytest.mark.parametrize("variant,K", VARIANT_K)
def test_hoisted_epilogue_forms_match_tile(dev, variant, K):
    """One row tile plus one row; N = 130 (partial-width lanes keep guarded loads, 16-byte prefetch through the padded
    leading dimension) for every form without statistics, N = 160 (one full and one partial column tile) for all."""
    BM = GEO[variant][0]
    for N in (130, 160):
        _compare(variant, _Case(dev, BM + 1, N, K), _forms(variant, N, K))


@pytest.mark.parametrize("variant", list(GEO))
def test_hoisted_epilogue_device_row_count(dev, variant):
    """A device row count whose last live tile has a single row (the clamp to row Mv - 1 of the hoisted prefetch), and
    a count of 0 (no tile is live: every output keeps its fill)."""
    BM, K = GEO[variant][0], 256
    for N in (130, 160):
        _compare(variant, _Case(dev, 3 * BM, N, K, m_dev=BM + 1), _forms(variant, N, K))
        _compare(variant, _Case(dev, 3 * BM, N, K, m_dev=0), _forms(variant, N, K), untouched=True)


@pytest.mark.parametrize("variant", list(GEO))
def test_hoisted_epilogue_seed_from_device_counter(dev, variant):
    """The dropout seed through the device counter (a dependent load, now in front of the loop): equal to the tile
    path at the same counter, and a different mask after the counter moved."""
    BM, K, N = GEO[variant][0], 192 if variant != "g8p" else 128, 160
    ctr = torch.full((1,), 5, dtype=torch.int64, device=dev)
    case = _Case(dev, BM + 1, N, K, counter=ctr)
    _compare(variant, case, ["rd", "rd_lns", "dgelu"])
    before = dict(case.launch("rd", GEO[variant][3]))["C"].clone()
    ops.counter_increment(ctr)
    _compare(variant, case, ["rd"])
    after = dict(case.launch("rd", GEO[variant][3]))["C"]
    torch.cuda.synchronize()
    assert not torch.equal(before, after)


@pytest.mark.parametrize("variant", list(GEO))
def test_hoisted_epilogue_f32_output(dev, variant):
    """fp32 C keeps the loads after the loop (no bf16 prefetch operand there): bias and bias + dropout forms."""
    BM, K, N = GEO[variant][0], 200, 130
    case = _Case(dev, BM + 1, N, K, c_dtype=torch.float32)
    for form, kw in (("bias", dict(bias=case.bias)), ("drop", dict(bias=case.bias, drop=case.drop, alpha=0.75))):
        out = {}
        for tile in (False, True):
            C = case.out()
            path = dict(tile_only=True) if tile else GEO[variant][3]
            names = _run(lambda: ops.gemm(case.A, case.B, C, split_k=1, **kw, **path))
            assert all(_is_native(variant, n) != tile for n in names), names
            out[tile] = C
        torch.cuda.synchronize()
        _assert_same(form, out[False], out[True])


@pytest.mark.parametrize("variant", [96, 160, 256])
def test_hoisted_epilogue_block_walks_two_tiles(dev, variant):
    """More live tiles than CUs: M = BM x (CUs + 3) at one column tile and one k-step, residual + dropout (+ the
    statistics producer) — a block runs a second tile and loads that tile's operands into the registers of the first."""
    BM, BN = GEO[variant][:2]
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    _compare(variant, _Case(dev, BM * (cus + 3), BN, 64), ["rd", "rd_lns"])


@pytest.mark.parametrize("variant", list(GEO))
def test_hoisted_epilogue_repeatable(dev, variant):
    """20 back-to-back launches of one residual + dropout + statistics product are bitwise identical."""
    BM, BN = GEO[variant][:2]
    case = _Case(dev, 2 * BM + 1, BN + 32, 320)
    first = dict(case.launch("rd_lns", GEO[variant][3]))
    outs = [dict(case.launch("rd_lns", GEO[variant][3])) for _ in range(20)]
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        for name in first:
            _assert_same(f"launch {i} {name}", o[name], first[name])
