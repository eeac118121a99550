"""fp64 references, per-element error weights and bounds for the training-time attention kernels
(csrc/attention_mfma.hip fwd v1 / v2 / v3, bwd v1 / v2 and their packed passes; csrc/attention.hip's VALU forward
with query tiling and VALU backward), the case list of their tests, a torch emulation of each arithmetic family's
rounding points and a Python restatement of the dispatch. Host only: nothing here touches a device.
test_attn_refs_cpu.py checks all of it without a GPU, test_attn_train_gpu.py checks the kernels against it.

Values. out, lse and dqkv are dropout_refs.attn_reference (autograd of ref_attention_drop; keep = None and p = 0
without dropout): one definition for the suite, a query with no allowed key has out = 0, lse = -inf and a zero
gradient. intermediates() restates the same in closed form (dV = Pd^T dO, dS = P (dPd - rowsum(P dPd)),
dQ = scale dS K, dK = scale dS^T Q) to get the weights below, and lse_reference is a hand-written fp64 logsumexp.

Weights (fp64; P the softmax, m the dropout scale keep / (1 - p) or 1, Pd = P m, G[q,k] = sum_d |dO[q,d]| |V[k,d]|):
    out[q,d]   A = sum_k Pd[q,k] |V[k,d]|
    dV[k,d]    A = sum_q Pd[q,k] |dO[q,d]|
    W[q,k]     = P[q,k] (m[q,k] G[q,k] + sum_k' P[q,k'] m[q,k'] G[q,k'])      (>= |dS[q,k]|)
    dQ[q,d]    A = scale sum_k W[q,k] |K[k,d]|
    dK[k,d]    A = scale sum_q W[q,k] |Q[q,d]|
    lse[q]     A = max over allowed k of scale sum_d |Q[q,d] K[k,d]|

The bound, per element: |got - ref| <= a |ref| + b A (lse: a (1 + |ref|) + b A, and -inf exactly where the reference is
-inf). Where A = 0 and ref = 0 the bound is 0: masked keys' dK / dV and a fully masked query's out / dQ must be exact
zeros. No element is left out. u = 2^-8 is bf16's unit roundoff (8 significant bits, round to nearest).

BOUNDS["mfma"] (fwd_kernel, fwd2_kernel, fwd3_kernel, bwd_kernel, bwd2_kernel; bf16 in and out):
    every output: a = u, the one bf16 rounding of the fp32 accumulator on store (f2bf / f2bf2).
    out: b = u. P (fwd v1 / v2: normalised, v3: exponentiated against the running max and divided by the sum after
        the product) is rounded to bf16 as the operand of the second MFMA product, a relative error of at most u on
        every term of the sum A bounds. What is fp32 — the score's accumulation over hd exact bf16 products
        (<= hd 2^-24 scale sum|q k|, 2e-4 at the peaked inputs), __expf's argument rounding (|x| 2^-24) and the
        accumulation over S terms — is a few percent of u and gets no allowance of its own: the two u terms are
        reached only if every rounding falls at its extreme with one sign.
    dV: b = u + 2^-12. The same u for Pd = exp(s - lse) m rounded to bf16; 2^-12 for the fp32 terms above plus the
        forward's lse, which the backward's P inherits.
    dQ, dK without O (bwd_kernel; "noO"): b = u + 2^-12. dS = P (dPd - delta) is rounded to bf16 as the second
        product's operand and |dS| <= W; delta = rowsum(P dPd) is an fp32 sum.
    dQ, dK with O (bwd2_kernel; BOUNDS["mfma_O"]): b = 2 u. u W for the rounding of dS as above. bwd2_kernel takes
        delta[q] = sum_d dO[q,d] O[q,d] from the forward's bf16 O, whose error is within u |O| + u A_out <= 2 u A_out
        per element, so |d delta| <= 2 u sum_k Pd G in the worst case, and it enters every dS[q,k] times P[q,k]: up
        to 2 u times the second term of W. That worst case needs all hd roundings of a row of O at their extreme
        and aligned in sign with dO; the bound allows half of it, u W, which also covers the fp32 terms.
    lse (every family): a = 2^-23 (m + logf(l) in fp32: logf within an ulp or two of log l, one rounding of the
        sum), b = 2^-17: the fp32 score accumulation, hd 2^-24 for the MFMA chain at hd <= 128 and (hd / 2 + 1) 2^-24
        for the VALU kernels' two accumulators at hd <= 160. A worst case again: observed ratios stay near 0.02.
BOUNDS["valu_bf16"] (attn_fwd_kernel<bf16>, attn_bwd_kernel<bf16>): fp32 throughout from bf16 inputs, one rounding
    of each output: a = u. b = 2^-13 for every output: P's relative error eps from the fp32 score accumulation
    ((hd / 2 + 1) 2^-24 scale sum|q k|, up to 1e-4 at the peaked inputs, where scale sum|q k| reaches 80) and __expf,
    plus S 2^-24 of accumulation. For dQ / dK the same eps serves: dS = P (dPd - delta) moves by eps |dS| directly
    and by eps P sum P|dPd| through delta (fp32 from P dPd: attn_bwd_kernel never reads O), together eps W.
BOUNDS["valu_f32"] (attn_fwd_kernel<float>, attn_bwd_kernel<float>): the same arithmetic without the output
    rounding: a = 2^-22, b as valu_bf16. These b are worst-case sums of fp32 roundings, sized for the peaked
    inputs; torch's fp32 and the device land one to two orders below them (roundings add like a random walk), so the
    fp32 ratios are small by construction. What the per-element form adds for fp32 is the small elements and the
    exact zeros; test_kernels_gpu.py's 1e-5 of the tensor's maximum stays in force beside it.
"""

import functools
import math

import torch

import dropout_refs as R

bf, f32 = torch.bfloat16, torch.float32
U = 2.0 ** -8
LDS_CAP = 160 * 1024

BOUNDS = {
    "mfma": dict(out=(U, U), dv=(U, U + 2.0 ** -12), dq=(U, U + 2.0 ** -12), dk=(U, U + 2.0 ** -12),
                 lse=(2.0 ** -23, 2.0 ** -17)),
    "valu_bf16": dict(out=(U, 2.0 ** -13), dv=(U, 2.0 ** -13), dq=(U, 2.0 ** -13), dk=(U, 2.0 ** -13),
                      lse=(2.0 ** -23, 2.0 ** -17)),
    "valu_f32": dict(out=(2.0 ** -22, 2.0 ** -13), dv=(2.0 ** -22, 2.0 ** -13), dq=(2.0 ** -22, 2.0 ** -13),
                     dk=(2.0 ** -22, 2.0 ** -13), lse=(2.0 ** -23, 2.0 ** -17)),
}
BOUNDS["mfma_O"] = dict(BOUNDS["mfma"], dq=(U, 2 * U), dk=(U, 2 * U))  # backward given O: bwd2_kernel
OUTPUTS = ("out", "lse", "dq", "dk", "dv")


def bounds(family, form="O"):
    """The (a, b) pairs of a family's outputs; form: the backward's, "O" (given the forward's output) or "noO"."""
    return BOUNDS["mfma_O"] if family == "mfma" and form == "O" else BOUNDS[family]


# ------------------------------------------------------------------------------------------------ dispatch


def rup(x, m):
    return (x + m - 1) // m * m


class Launch:
    """What the dispatch reads of a call besides (dtype, hd, S): leading dimensions in elements, the out pointer's
    address modulo 16 (every other pointer is 16-byte aligned in these tests) and whether the backward is given O."""

    def __init__(self, ld_qkv, ld_out, ld_dout=None, ld_dqkv=None, out_mod16=0, out_given=True):
        self.ld_qkv, self.ld_out, self.ld_dout, self.ld_dqkv = ld_qkv, ld_out, ld_dout, ld_dqkv
        self.out_mod16, self.out_given = out_mod16, out_given


def ldr_of(hd):
    return hd + 16


def mfma_fwd_lds(S, hd):
    ldT = rup(S, 32) + 8
    return 2 * (hd * ldT + 4 * 16 * ldT)


def mfma_bwd_lds(S, hd):
    ldT = rup(S, 32) + 8
    return 2 * (3 * hd * ldT + 2 * rup(S, 16) * ldT + 4 * 16 * ldT)


def mfma_bwd2_lds(S, hd):
    return 2 * (3 * rup(S, 32) + rup(S, 16)) * ldr_of(hd) + 2 * 4 * rup(S, 32) + rup(S, 32)


def mfma_fwd3_lds(S, hd):
    return 2 * 2 * rup(S, 32) * ldr_of(hd)


def mfma_fwd2_ok(dtype, hd, S, l):
    if l.ld_out & 3 or l.ld_qkv & 7 or l.out_mod16 & 7:
        return False
    return rup(S, 16) // 16 * 64 <= 512


def mfma_bwd2_ok(dtype, hd, S, l):
    if not l.out_given or l.ld_out & 7 or l.ld_dqkv & 7 or l.out_mod16 & 15:
        return False
    return rup(S, 16) // 16 * 64 <= 512 and mfma_bwd2_lds(S, hd) <= LDS_CAP


def mfma_fwd3_ok(dtype, hd, S, l):
    if dtype != bf or hd not in (64, 96) or S <= 128:
        return False
    if l.ld_out & 3 or l.ld_qkv & 7 or l.out_mod16 & 7:
        return False
    return mfma_fwd3_lds(S, hd) <= LDS_CAP


def mfma_attention_ok(dtype, hd, S, l, bwd):
    if not bwd and mfma_fwd3_ok(dtype, hd, S, l):
        return True
    if dtype == bf and hd == 128 and S <= 128 and not l.ld_qkv & 7:
        return (not l.ld_dout & 7 and mfma_bwd2_ok(dtype, hd, S, l)) if bwd else mfma_fwd2_ok(dtype, hd, S, l)
    if dtype != bf or hd not in (64, 96) or S > 128:
        return False
    if l.ld_qkv & 7 or (bwd and l.ld_dout & 7):
        return False
    if bwd:
        return mfma_bwd2_ok(dtype, hd, S, l) or mfma_bwd_lds(S, hd) <= LDS_CAP
    return mfma_fwd_lds(S, hd) <= LDS_CAP


def valu_fwd_lds(S, hd, QT):
    return 4 * ((2 * S + QT) * (hd + 1) + QT * S)


def valu_bwd_lds(S, hd):
    return 4 * (4 * S * (hd + 1) + 2 * S * S)


def fwd_rows(S, hd):
    if valu_fwd_lds(S, hd, S) <= LDS_CAP:
        return S
    qt = 128
    while qt >= 4:
        if qt < S and valu_fwd_lds(S, hd, qt) <= LDS_CAP:
            return qt
        qt >>= 1
    return 0


def select(dtype, hd, S, l, bwd):
    """The kernel icap_attention_fwd / icap_attention_bwd launch for this call, by name (None: refused).
    mfma_attention_launch's order: forward v3, v2, v1; backward v2, v1; else the VALU kernels of attention.hip.
    A restatement kept in step with csrc/attention_mfma.hip and csrc/attention.hip by hand: a gate changed there
    alone is not seen here, only by the GPU cases that then meet another kernel's behaviour (or a refusal). The
    qkv / dout / dqkv pointer checks (& 15) of the C++ gates are left out: every such pointer in these tests is a
    fresh allocation, 16-byte aligned (asserted in test_attn_train_gpu.py)."""
    t = "bf16" if dtype == bf else "float"
    if mfma_attention_ok(dtype, hd, S, l, bwd):
        if not bwd:
            if mfma_fwd3_ok(dtype, hd, S, l):
                return f"fwd3_kernel<{hd}>"
            return f"fwd2_kernel<{hd}>" if mfma_fwd2_ok(dtype, hd, S, l) else f"fwd_kernel<{hd}>"
        return f"bwd2_kernel<{hd}>" if mfma_bwd2_ok(dtype, hd, S, l) else f"bwd_kernel<{hd}>"
    if bwd:
        return f"attn_bwd_kernel<{t}>" if valu_bwd_lds(S, hd) <= LDS_CAP else None
    QT = fwd_rows(S, hd)
    if QT == 0:
        return None
    return f"attn_fwd_kernel<{t}>" + ("" if QT == S else f" QT={QT} chunks={-(-S // QT)} last={S - (-(-S // QT) - 1) * QT}")


def packed_passes(S, short_only):
    """mfma_attention_launch's passes over a packed launch of S tokens (packed_split / SHORT_S = 32)."""
    if S <= 32:
        return ("single",)
    return ("short",) if short_only else ("short", "long")


# ------------------------------------------------------------------------------------------------ cases

PAD = 8  # pad columns of the out / dqkv buffers (keeps every row 16-byte aligned in both dtypes)


class Case:
    """One forward (out, lse) and its backwards. B = 2, H = 3 so batch and head indexing both matter.
    family: key of BOUNDS. forms: backward forms run, of "O" (out given) and "noO". off2: out is the 4-byte-aligned
    view buf[:, 2:2+D] (the second-generation forward does not take it). big: q and k scaled by 3 (peaked softmax).
    masked: the ragged key mask of dropout_refs.AttnCase; hide0: key 0 of batch row 1 hidden (with causal its
    query 0 has no allowed key). expect: {"fwd" / "O" / "noO": kernel name}, pinned by test_attn_refs_cpu.py."""

    B, H, p, keep = 2, 3, 0.0, None

    def __init__(self, name, family, dtype, hd, S, causal, masked, forms=("O",), big=False, hide0=False, off2=False,
                 expect=None):
        self.name, self.family, self.dtype, self.hd, self.S = name, family, dtype, hd, S
        self.causal, self.masked, self.forms, self.big, self.hide0, self.off2 = causal, masked, forms, big, hide0, off2
        self.scale = 1.0 / math.sqrt(hd)
        self.expect = expect or {}

    def __repr__(self):
        return self.name

    def key_mask(self):
        if not (self.masked or self.hide0):
            return None
        km = torch.ones((self.B, self.S), dtype=torch.int32)
        if self.masked:
            km[0, max(self.S - 3, 0):] = 0   # (S <= 3: batch row 0 has no allowed key at all)
            km[1, self.S // 2:] = 0
        if self.hide0:
            km[1, 0] = 0
        return km

    def inputs(self):
        """(qkv [B*S, 3D], dout [B*S, D]) in the case's dtype (CPU), N(0,1) from a per-case seed."""
        D = self.H * self.hd
        seed = 1000 * self.hd + 2 * self.S + (1 if self.causal else 0)
        qkv = R.randn((self.B * self.S, 3 * D), 7_000_000 + seed)
        if self.big:
            qkv[:, :2 * D] *= 3
        return qkv.to(self.dtype), R.randn((self.B * self.S, D), 8_000_000 + seed).to(self.dtype)

    def launch(self, form="O"):
        D = self.H * self.hd
        return Launch(3 * D, D + PAD, D, 3 * D + PAD, out_mod16=4 if self.off2 else 0, out_given=form == "O")

    def selected(self):
        d = {"fwd": select(self.dtype, self.hd, self.S, self.launch(), False)}
        for f in self.forms:
            d[f] = select(self.dtype, self.hd, self.S, self.launch(f), True)
        return d


def _both(prefix, family, dtype, hd, S, forms, expect, **kw):
    """causal + ragged key mask ("cm"), and non-causal without a mask ("plain")."""
    return [Case(f"{prefix}-S{S}-cm", family, dtype, hd, S, True, True, forms, expect=expect, **kw),
            Case(f"{prefix}-S{S}-plain", family, dtype, hd, S, False, False, forms, expect=expect, **kw)]


def _v2(hd):
    return {"fwd": f"fwd2_kernel<{hd}>", "O": f"bwd2_kernel<{hd}>"}


V2_S64 = (1, 15, 16, 17, 31, 32, 33, 48, 49, 64, 65, 96, 97, 112, 113, 127, 128)
V2_S = (16, 17, 33, 49, 65, 97, 113, 128)
CASES = []
for _S in V2_S64:
    CASES += _both("v2-64", "mfma", bf, 64, _S, ("O",), _v2(64))
for _hd in (96, 128):
    for _S in V2_S:
        CASES += _both(f"v2-{_hd}", "mfma", bf, _hd, _S, ("O",), _v2(_hd))
for _hd in (64, 96, 128):
    for _S in (65, 128):
        CASES.append(Case(f"v2-{_hd}-S{_S}-cm-big", "mfma", bf, _hd, _S, True, True, ("O",), big=True,
                          expect=_v2(_hd)))
# first-generation backward (out=None); hd 96 stops at 112, where its LDS image fits
for _hd, _Ss in ((64, (17, 49, 65, 112, 128)), (96, (17, 49, 65, 112))):
    for _S in _Ss:
        CASES += _both(f"v1bwd-{_hd}", "mfma", bf, _hd, _S, ("noO",),
                       {"fwd": f"fwd2_kernel<{_hd}>", "noO": f"bwd_kernel<{_hd}>"})
# first-generation forward through the 4-byte-aligned out view
for _hd in (64, 96):
    for _S in (17, 65, 128):
        CASES += _both(f"v1fwd-{_hd}", "mfma", bf, _hd, _S, (), {"fwd": f"fwd_kernel<{_hd}>"}, off2=True)
# long-sequence forward: 512 / 352 are the largest S each head dim's LDS image admits; 257 at hd 64 is 17 query
# tiles in 2 passes of 9 waves
for _hd, _Ss in ((64, (129, 144, 145, 257, 512)), (96, (129, 257, 352))):
    for _S in _Ss:
        CASES += _both(f"v3-{_hd}", "mfma", bf, _hd, _S, (), {"fwd": f"fwd3_kernel<{_hd}>"})
CASES.append(Case("v3-64-S145-hide0", "mfma", bf, 64, 145, True, False, (), hide0=True, big=True,
                  expect={"fwd": "fwd3_kernel<64>"}))
# VALU fp32: forward + backward up to S = 92, the largest the backward's LDS formula admits at hd 64
_VF = {"fwd": "attn_fwd_kernel<float>", "O": "attn_bwd_kernel<float>"}
for _S in (1, 33, 65, 92):
    CASES += _both("valu-f32-64", "valu_f32", f32, 64, _S, ("O",), _VF)
CASES.append(Case("valu-f32-64-S65-cm-big", "valu_f32", f32, 64, 65, True, True, ("O",), big=True, expect=_VF))
# forward alone: 127 is the largest one-chunk forward; then query tiling with a short last chunk
for _S, _e in ((127, "attn_fwd_kernel<float>"), (128, "attn_fwd_kernel<float> QT=64 chunks=2 last=64"),
               (197, "attn_fwd_kernel<float> QT=32 chunks=7 last=5"),
               (257, "attn_fwd_kernel<float> QT=16 chunks=17 last=1")):
    CASES += _both("valu-f32-64", "valu_f32", f32, 64, _S, (), {"fwd": _e})
# bf16 at head dims the MFMA gate rejects
_VB = {"fwd": "attn_fwd_kernel<bf16>", "O": "attn_bwd_kernel<bf16>", "noO": "attn_bwd_kernel<bf16>"}
CASES += _both("valu-bf16-16", "valu_bf16", bf, 16, 9, ("O", "noO"), _VB)
CASES += _both("valu-bf16-160", "valu_bf16", bf, 160, 25, ("O", "noO"), _VB)

# every kernel the case list must reach (test_attn_refs_cpu.py test_dispatch_table)
KERNELS = ([f"fwd2_kernel<{h}>" for h in (64, 96, 128)] + [f"bwd2_kernel<{h}>" for h in (64, 96, 128)] +
           [f"fwd_kernel<{h}>" for h in (64, 96)] + [f"bwd_kernel<{h}>" for h in (64, 96)] +
           [f"fwd3_kernel<{h}>" for h in (64, 96)] +
           ["attn_fwd_kernel<float>", "attn_fwd_kernel<float> QT=64 chunks=2 last=64",
            "attn_fwd_kernel<float> QT=32 chunks=7 last=5", "attn_fwd_kernel<float> QT=16 chunks=17 last=1",
            "attn_bwd_kernel<float>", "attn_fwd_kernel<bf16>", "attn_bwd_kernel<bf16>"])


class DropCase:
    """A dropout_refs.AttnCase (B = 2, H = 2, its own inputs and device mask) under the per-element bound."""

    def __init__(self, case, family, forms):
        self.c, self.family, self.forms, self.name = case, family, forms, "drop-" + case.name
        for k in ("dtype", "B", "H", "S", "hd", "causal", "scale", "p"):
            setattr(self, k, getattr(case, k))
        self.off2 = False
        d, ctr = case.desc()
        self.keep = R.attn_keep(d, case.B, case.H, case.S, ctr)

    def __repr__(self):
        return self.name

    def key_mask(self):
        return self.c.key_mask()

    def inputs(self):
        return self.c.inputs()


def _drop(name):
    return next(c for c in R.ATTN_CASES + R.HIDE0_CASES if c.name == name)


DROP_CASES = [DropCase(_drop("v2-64-S65-p.5"), "mfma", ("O", "noO")), DropCase(_drop("v2-96-S25"), "mfma", ("O", "noO")),
              DropCase(_drop("v3-64-S257"), "mfma", ()), DropCase(_drop("valu-f32-S65"), "valu_f32", ("O",)),
              DropCase(_drop("hide0-v2-64-S33"), "mfma", ("O", "noO")), DropCase(_drop("hide0-v3-64-S129"), "mfma", ())]


class PackedCase:
    """Packed sequences (seqs=): sequence b has lens[b] <= S tokens at packed rows off[b] + t, one hidden key;
    causal as the caption batches are, and once without (only then can a key past the sequence's end be reached).
    The reference is the padded problem [B, S] with key_mask = (t < lens[b]) and zero dO on dead rows; only
    live rows are compared (and lse only at q < lens[b], the positions a packed launch writes: include/icap.h)."""

    H, p, keep, off2 = 3, 0.0, None, False

    def __init__(self, name, family, dtype, hd, S, lens, short_only=False, hole=None, causal=True):
        self.name, self.family, self.dtype, self.hd, self.S, self.lens = name, family, dtype, hd, S, tuple(lens)
        self.short_only, self.hole, self.B, self.forms, self.causal = short_only, hole, len(lens), ("O",), causal
        self.scale = 1.0 / math.sqrt(hd)
        self.off = tuple(int(sum(lens[:b])) for b in range(self.B))
        self.n = int(sum(lens))

    def __repr__(self):
        return self.name

    def key_mask(self):
        km = torch.zeros((self.B, self.S), dtype=torch.int32)
        for b, n in enumerate(self.lens):
            km[b, :n] = 1
        if self.hole is not None:
            km[self.hole] = 0
        return km

    def live_rows(self):
        """padded row index b*S + t of packed row i, for i < n."""
        return torch.cat([torch.arange(b * self.S, b * self.S + n) for b, n in enumerate(self.lens)] +
                         [torch.zeros(0, dtype=torch.int64)])

    def live_lse(self):
        """index into lse [B, H, S] of the entries a packed launch writes."""
        idx = torch.arange(self.B * self.H * self.S).view(self.B, self.H, self.S)
        return torch.cat([idx[b, :, :n].reshape(-1) for b, n in enumerate(self.lens)])

    def inputs(self):
        """padded (qkv [B*S, 3D], dout [B*S, D]); dout is zero on dead rows."""
        D = self.H * self.hd
        qkv = R.randn((self.B * self.S, 3 * D), 9_000_000 + self.S + len(self.lens)).to(self.dtype)
        dout = torch.zeros((self.B * self.S, D), dtype=self.dtype)
        rows = self.live_rows()
        dout[rows] = R.randn((self.n, D), 9_100_000 + self.S).to(self.dtype)
        return qkv, dout


PACKED_CASES = [
    PackedCase("packed-64-S65", "mfma", bf, 64, 65, (0, 1, 16, 17, 32, 33, 65), hole=(5, 2)),
    PackedCase("packed-64-S32", "mfma", bf, 64, 32, (1, 32), hole=(1, 7)),
    PackedCase("packed-64-S65-short_only", "mfma", bf, 64, 65, (0, 1, 16, 17, 32, 5, 31), short_only=True, hole=(4, 2)),
    PackedCase("packed-f32-64-S65", "valu_f32", f32, 64, 65, (0, 5, 65), hole=(2, 7)),
    PackedCase("packed-64-S65-noncausal", "mfma", bf, 64, 65, (5, 33, 16, 40), hole=(3, 2), causal=False),
    PackedCase("packed-f32-64-S65-noncausal", "valu_f32", f32, 64, 65, (5, 33), hole=(1, 2), causal=False),
]


# ------------------------------------------------------------------------------------------------ references


def heads(x, B, S, H, hd):
    """[B*S, H*hd] -> [B, H, S, hd]"""
    return x.view(B, S, H, hd).permute(0, 2, 1, 3)


def rows(x):
    """[B, H, S, hd] -> [B*S, H*hd]"""
    B, H, S, hd = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * S, H * hd)


def lse_reference(q, k, scale, allowed):
    """fp64 logsumexp of the allowed scaled scores, written out: max + log(sum exp(s - max)); -inf where no key is
    allowed. q, k: [B, H, S, hd] fp64; allowed: bool, broadcastable to [B, H, S, S]."""
    s = ((q @ k.transpose(-1, -2)) * scale).masked_fill(~allowed, float("-inf"))
    mx = s.amax(-1, keepdim=True)
    safe = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)
    l = torch.exp(s - safe).sum(-1, keepdim=True)
    return torch.where(l > 0, safe + torch.log(l.clamp_min(1e-300)), torch.full_like(l, float("-inf"))).squeeze(-1)


def intermediates(qkv, dout, B, S, H, hd, scale, causal, key_mask, keep, p, allowed=None):
    """Closed-form fp64 attention and the error weights of the module docstring. Returns a dict: out, dq, dk, dv and
    A_out, A_dq, A_dk, A_dv as [B*S, D]; lse, A_lse as [B*H*S] (the d* entries only with dout).
    allowed: overrides the mask rule (bool [B, H or 1, S, S]; the reference-side mutants)."""
    x = qkv.double().view(B, S, 3, H, hd).permute(2, 0, 3, 1, 4)
    q, k, v = x[0], x[1], x[2]
    if allowed is None:
        allowed = R.allowed_mask(B, S, causal, key_mask)
    s = ((q @ k.transpose(-1, -2)) * scale).masked_fill(~allowed, float("-inf"))
    live = allowed.any(-1, keepdim=True)
    P = torch.softmax(torch.where(live, s, torch.zeros_like(s)), -1) * live
    m = torch.ones_like(P) if keep is None else keep.double() * R.inv_keep(p)
    Pd = P * m
    r = dict(out=rows(Pd @ v), A_out=rows(Pd @ v.abs()), lse=lse_reference(q, k, scale, allowed).reshape(-1),
             A_lse=((q.abs() @ k.abs().transpose(-1, -2)) * scale).masked_fill(~allowed, 0.0).amax(-1).reshape(-1))
    if dout is not None:
        dO = heads(dout.double(), B, S, H, hd)
        dPd = (dO @ v.transpose(-1, -2)) * m
        dS = P * (dPd - (P * dPd).sum(-1, keepdim=True))
        G = dO.abs() @ v.abs().transpose(-1, -2)
        W = P * (m * G + (P * m * G).sum(-1, keepdim=True))
        r.update(dv=rows(Pd.transpose(-1, -2) @ dO), A_dv=rows(Pd.transpose(-1, -2) @ dO.abs()),
                 dq=rows(dS @ k) * scale, A_dq=rows(W @ k.abs()) * scale,
                 dk=rows(dS.transpose(-1, -2) @ q) * scale, A_dk=rows(W.transpose(-1, -2) @ q.abs()) * scale)
    return r


@functools.lru_cache(maxsize=None)
def reference(case):
    """The fp64 reference of a case and its weights: dict with out, lse, dq, dk, dv (values: dropout_refs.
    attn_reference) and A_out, A_lse, A_dq, A_dk, A_dv. Computed once per case; callers must not modify it."""
    qkv, dout = case.inputs()
    g = (case.B, case.S, case.H, case.hd, case.scale, case.causal, case.key_mask(), case.keep, case.p)
    r = intermediates(qkv, dout, *g)
    o, lse, dqkv = R.attn_reference(qkv, dout, *g)
    D = case.H * case.hd
    r.update(out=o, lse=lse, dq=dqkv[:, :D], dk=dqkv[:, D:2 * D], dv=dqkv[:, 2 * D:])
    return r


def ratio(got, ref, A, ab, lse=False):
    """max over every element of |got - ref| / (a |ref| + b A) (lse: a (1 + |ref|) + b A); inf where the bound is 0
    and the error is not (exact zeros), or where got and ref are not -inf at the same places; nan if got has one."""
    a, b = ab
    got, ref, A = got.detach().double().cpu(), ref.double(), A.double()
    assert got.shape == ref.shape == A.shape, (got.shape, ref.shape, A.shape)
    if got.numel() == 0:
        return 0.0
    if torch.isnan(got).any():
        return float("nan")
    if lse:
        ninf = ref == float("-inf")
        if not torch.equal(got == float("-inf"), ninf):
            return float("inf")
        got, ref, A = got[~ninf], ref[~ninf], A[~ninf]
        if got.numel() == 0:
            return 0.0
        bound = a * (1 + ref.abs()) + b * A
    else:
        bound = a * ref.abs() + b * A
    err = (got - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).double())
    return r.max().item()


def ratios(family, got, ref, sel=None, lse_sel=None, form="O"):
    """{output: ratio} for the outputs present in `got` (keys of OUTPUTS) under bounds(family, form). sel / lse_sel: (index into got's rows,
    index into the reference's rows) for the packed cases' live rows and written lse entries."""
    out = {}
    for k in OUTPUTS:
        if k not in got:
            continue
        g, r, A = got[k], ref[k], ref["A_" + k]
        s = lse_sel if k == "lse" else sel
        if s is not None:
            g, r, A = g[s[0]], r[s[1]], A[s[1]]
        out[k] = ratio(g, r, A, bounds(family, form)[k], lse=k == "lse")
    return out


# ------------------------------------------------------------------------------------------------ emulation


def emulate(case, form="O"):
    """The case in torch fp32 with the family's rounding points (CPU test only): mfma — Pd and dS rounded to bf16
    before the second product, outputs rounded once, delta from the rounded O (form "O") or from P dPd in fp32
    ("noO"); valu_bf16 — fp32 throughout (delta from P dPd: attn_bwd_kernel never reads O), outputs rounded once;
    valu_f32 — fp32 throughout. The backward takes
    P = exp(s - lse) from the emulated forward's fp32 lse, as the kernels do. Returns the dict ratios() reads."""
    B, S, H, hd, scale = case.B, case.S, case.H, case.hd, case.scale
    qkv, dout = case.inputs()
    x = qkv.float().view(B, S, 3, H, hd).permute(2, 0, 3, 1, 4)
    q, k, v = x[0], x[1], x[2]
    mf = case.family == "mfma"
    rb = (lambda t: t.to(bf).float()) if mf else (lambda t: t)
    ro = lambda t: t.to(case.dtype).float()  # noqa: E731
    allowed = R.allowed_mask(B, S, case.causal, case.key_mask())
    s = ((q @ k.transpose(-1, -2)) * torch.tensor(scale, dtype=f32)).masked_fill(~allowed, float("-inf"))
    mx = s.amax(-1, keepdim=True)
    live = ~torch.isinf(mx)
    safe = torch.where(live, mx, torch.zeros_like(mx))
    e = torch.exp(s - safe) * live
    l = e.sum(-1, keepdim=True)
    lse = torch.where(live, safe + torch.log(l.clamp_min(1e-30)), torch.full_like(l, float("-inf")))
    m = torch.ones_like(e) if case.keep is None else case.keep.float() * torch.tensor(1.0, dtype=f32) / (
        1 - torch.tensor(case.p, dtype=f32))
    P = e / l.clamp_min(1e-30)
    o = ro(rb(P * m) @ v)
    r = dict(out=rows(o), lse=lse.reshape(-1))
    dO = heads(dout.float(), B, S, H, hd)
    Pb = torch.where(allowed & live, torch.exp(s - torch.where(live, lse, torch.zeros_like(lse))), torch.zeros_like(s))
    dPd = (dO @ v.transpose(-1, -2)) * m
    delta = (dO * o).sum(-1, keepdim=True) if mf and form == "O" else (Pb * dPd).sum(-1, keepdim=True)
    dS = rb(Pb * (dPd - delta))
    sc = torch.tensor(scale, dtype=f32)
    r.update(dv=rows(ro(rb(Pb * m).transpose(-1, -2) @ dO)), dq=rows(ro((dS @ k) * sc)),
             dk=rows(ro((dS.transpose(-1, -2) @ q) * sc)))
    return r
