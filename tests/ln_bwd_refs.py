"""fp64 reference (CPU tensors), cases and bounds of the LayerNorm backward (icap_layernorm_bwd and the batched
parameter reduce icap_ln_param_reduce_batch). test_ln_bwd_refs_cpu.py checks the reference and the bounds on
their own without a GPU (the formula against torch.autograd, a plain fp32 evaluation inside every bound, a list of
deliberately wrong results outside), test_ln_bwd_gpu.py checks the kernels against them. The "reaches" strings
of the cases are read from the dispatch in csrc/layernorm.hip icap_layernorm_bwd (restated in `reaches()`), not
observed.

Inputs are dropout_refs.LnCase.inputs() of the same (rows, D). Rows past `live` (the device row count rows_dev)
of x and dres are NaN, and so is every dy row that no live row gathers (without a row map: the rows past `live`;
with one, the targets of the dead rows and of nothing), so anything read from them poisons dx or the parameter
sums. mean and rstd are computed here, in fp64 from the case's (bf16- or fp32-valued) x, rounded to fp32 and used
in that form by the kernel AND by the reference: the backward is tested on its own and the rounding of the
statistics does not enter the bound.

Reference (a formula, not autograd), xh = (x - mean) * rstd, dy' = dy gathered through the row map (zero where
the map is < 0), gy = dy' * gamma, mean_c the mean over the D columns:

    dx     = rstd * (gy - mean_c(gy) - xh * mean_c(gy * xh)) + dres
    dgamma = sum_r dy' * xh  (+ the initial gradient when accumulating),   dbeta = sum_r dy'    (live rows only)

Bounds, U = 2^-24, r16 = 2^-8 for bf16 (the one rounding of the stored element), 0 for fp32:

    dx per element      |d| <= r16 * |ref| + K_DX * U * A,
                        A = rstd * (|gy| + mean_c|gy| + |xh| * mean_c|gy * xh|) + |dres|
    dgamma per column   |d| <= K_P * U * (sum_r |dy' * xh| + |initial|)
    dbeta per column    |d| <= K_P * U * (sum_r |dy'|      + |initial|)

A is the size of the terms before they cancel, with the row means of ABSOLUTE values: the two row sums are off by
ulps of mean|gy|, not of |m1|. Where A (or a column's sum) is zero the bound is zero and the result must be the
reference exactly (a dead call's dgamma = 0). dx_drop = dx * keep / (1 - p) has the same bound scaled by
1 / (1 - p) with K_DX + 2: the fp32 rounding of the scale and of the product.

The constants are not tuned against the kernel: they come from torch's plain fp32 evaluation of the same formula
on the CPU (ln_bwd_fp32) over ALL cases below, the next power of two at or above 4 x the worst ratio seen with
K = 1 (the margin loss_refs.py uses for cross entropy; it is there because the kernel sums in another order and
contracts to FMA). Measured (error / (U * A) for fp32 cases; bf16 cases measured on the fp32 value before its
rounding):
    dx      worst 2.79 (32777 x 64 fp32, no parameters); 0.98 at 9 x 4, 1.94 at 9 x 768 bf16, 2.14 at 9 x 1536
            fp32, 2.29 at 32777 x 64 bf16                                         -> 4 x = 11.2 -> K_DX = 16
    dgamma  worst 3.68 (9 x 1020 fp32), dbeta worst 2.84 (9 x 1288 fp32); at 2057 rows 0.19 .. 0.27 and <= 0.21
            (a 9-row sum of bf16 values is exact in fp32: dbeta 0 there)          -> 4 x = 14.7 -> K_P  = 16
(test_ln_bwd_refs_cpu.py test_constants_follow_the_fp32_measurement recomputes both and asserts the rule.)

Every check function returns the worst ratio of error to bound it saw (<= 1 passes), so a test can print it.
"""

import functools
import math

import torch

from dropout_refs import LnCase, inv_keep, make_desc, randn, site_keep
from loss_refs import LN_EPS, SENTINEL, dt_name, f32r

bf, f32 = torch.bfloat16, torch.float32
U = 2.0 ** -24
K_DX = 16.0
K_P = 16.0
LN_BWD_BLOCKS = 256     # csrc/layernorm.hip: the grid cap of a call with dgamma / dbeta (4096 without)
NAN = float("nan")


def chunks(D):
    return 3 if D <= 768 else 4 if D <= 1024 else 5 if D <= 1280 else 6


class LnBwdCase:
    """x [rows, D] (row stride ldx, based x_off elements into a 16-byte aligned buffer), dy (lddy), dres (lddres,
    or none), dx and dx_drop (lddx). dgamma / dbeta: which parameter gradients are asked for; accumulate: += onto
    a non-zero gradient, else = onto NaN. live: rows_dev (None: none). rowmap: dy_rowmap (LnCase.inputs()).
    drop_p > 0: dx_drop is asked for."""

    def __init__(self, name, dtype, rows, D, dres=True, dgamma=True, dbeta=True, accumulate=False, live=None,
                 rowmap=False, ldx=None, lddy=None, lddres=None, lddx=None, x_off=0, drop_p=0.0, big=False):
        self.name, self.dtype, self.rows, self.D = name, dtype, rows, D
        self.dres, self.dgamma, self.dbeta, self.accumulate = dres, dgamma, dbeta, accumulate
        self.rows_dev, self.rowmap, self.x_off, self.drop_p, self.big = live, rowmap, x_off, drop_p, big
        self.live = rows if live is None else live
        self.ldx, self.lddy, self.lddres, self.lddx = ldx or D, lddy or D, lddres or D, lddx or D
        self.params = dgamma or dbeta
        self.reaches = reaches(self)

    def __repr__(self):
        return self.name

    def base(self):
        return LnCase(self.name, self.dtype, self.rows, self.D, p=self.drop_p, big=self.big, dres=self.dres,
                      rowmap=self.rowmap)

    @functools.lru_cache(maxsize=None)
    def inputs(self):
        """x, dy, dres (or None) [rows, D] in the case's dtype with the NaN rows of the module docstring, gamma
        [D], rowmap int32 [rows] (or None), mean / rstd fp32 [rows] (NaN past `live`), gather int64 [live]: the dy
        row of live row r (negative: zero), dgamma0 / dbeta0 [D]: what the gradients hold before the call."""
        t = self.base().inputs()
        n, rows = self.live, self.rows
        x, dy = t["x"].clone(), t["dy"].clone()
        x[n:] = NAN
        rm = t["rowmap"]
        gather = torch.arange(n) if rm is None else rm[:n].long()
        used = torch.zeros(rows, dtype=torch.bool)
        used[gather[gather >= 0]] = True
        dy[~used] = NAN
        dres = None
        if t["dres"] is not None:
            dres = t["dres"].clone()
            dres[n:] = NAN
        xd = x[:n].double()
        mean = xd.mean(1)
        rstd = 1.0 / torch.sqrt(((xd - mean[:, None]) ** 2).mean(1) + f32r(LN_EPS))
        stats = torch.full((2, rows), NAN, dtype=f32)
        stats[0, :n], stats[1, :n] = mean.float(), rstd.float()
        if self.accumulate:
            g0, b0 = randn((self.D,), 18) * 0.5 + 1.0, randn((self.D,), 19) * 0.5 - 1.0
        else:
            g0 = b0 = torch.full((self.D,), NAN)
        return dict(x=x, dy=dy, dres=dres, gamma=t["gamma"], rowmap=rm, mean=stats[0], rstd=stats[1],
                    gather=gather, dgamma0=g0, dbeta0=b0)

    def keep(self):
        """bool [rows, D]: dx_drop's mask, element (r, c) at index offset + r * D + c whatever lddx is."""
        d, ctr = make_desc(self.drop_p, self.big)
        return site_keep(d, (self.rows, self.D), ctr)


def reaches(c):
    """icap_layernorm_bwd's dispatch restated: the 8-wide form needs D % 8 == 0 and, for every one of x, dy, dx,
    dres and dx_drop that is given, a stride that is a multiple of 8 and a 16-byte aligned base (only x is ever
    based off the buffer's start here); any one that is not sends the call to the 4-wide kernel."""
    es = 2 if c.dtype == bf else 4
    strides = [c.ldx, c.lddy, c.lddx] + ([c.lddres] if c.dres else [])
    wide = c.D % 8 == 0 and all(s % 8 == 0 for s in strides) and (c.x_off * es) % 16 == 0
    if wide:
        return f"ln_bwd8_kernel<{dt_name(c.dtype)}, {'true' if c.params else 'false'}, {chunks(c.D)}>"
    return f"ln_bwd_kernel<{dt_name(c.dtype)}>"


def launch(c):
    """(blocks, rows per pass, passes, blocks that own no row) of the launch, restated from icap_layernorm_bwd:
    ceil(rows / 4) blocks capped at 256 with parameters for BOTH forms (the workspace is sized for it), and
    without them ceil(rows / 8) or ceil(rows / 4) capped at 4096; 8 or 4 rows per block."""
    wide = c.reaches.startswith("ln_bwd8")
    per = 8 if wide else 4
    nb = min(-(-c.rows // 4), LN_BWD_BLOCKS) if c.params else min(-(-c.rows // per), 4096)
    nb = max(nb, 1)
    return nb, nb * per, -(-c.live // (nb * per)), max(0, nb - -(-c.live // per))


def _c(rows, D, dt, **kw):
    tag = "".join("-" + (k if v is True else f"no{k}" if v is False else f"{k}{v}") for k, v in kw.items())
    return LnBwdCase(f"{rows}x{D}-{dt_name(dt)}{tag}", dt, rows, D, **kw)


NOPARAMS = dict(dgamma=False, dbeta=False)
LN8_D = [8, 256, 512, 768, 776, 1024, 1032, 1280, 1288, 1536]   # 776 / 1032 / 1288: first D of the 4 / 5 / 6 chunks
LN4_D = [4, 132, 1020]                                          # 1020: all four float4 groups live
BOTH = (bf, f32)

# 9 rows at every width class, with parameters and dres; then PARAMS = false, the dtypes alternating so that both
# reach each of the four chunk counts
CASES = [_c(9, D, dt) for D in LN8_D + LN4_D for dt in BOTH]
CASES += [_c(9, D, BOTH[i % 2], **NOPARAMS) for i, D in enumerate(LN8_D + LN4_D)]
# row counts: 12 rows make the 8-wide launch 3 blocks of which the last owns no row (37: 10 blocks, 5 empty)
CASES += [_c(r, D, dt) for r in (1, 7, 8, 12, 37) for D in (768, 132) for dt in BOTH]
# past the grid caps: the row loops take a second pass (ln_bwd_kernel prefetches its row across the passes)
CASES += [c for dt in BOTH for c in (
    _c(2057, 64, dt), _c(2057, 64, dt, rowmap=True, accumulate=True),
    _c(1029, 36, dt), _c(1029, 36, dt, rowmap=True, accumulate=True),
    _c(32777, 64, dt, **NOPARAMS), _c(16389, 36, dt, **NOPARAMS),
)]
# strides and alignment
CASES += [c for dt in BOTH for c in (
    _c(9, 768, dt, lddy=776), _c(9, 768, dt, lddres=776), _c(9, 768, dt, lddx=776),      # 8-wide, padding survives
    _c(9, 768, dt, lddy=776, lddres=784, lddx=792),                                    # three unlike strides
    _c(9, 768, dt, lddy=772), _c(9, 768, dt, lddres=772), _c(9, 768, dt, lddx=772),      # any one: 4-wide
    _c(9, 768, dt, ldx=772),
    _c(9, 768, dt, x_off=4),                                # bf16: 8 bytes in, 4-wide; fp32: 16 bytes in, 8-wide
    _c(9, 768, dt, lddx=776, drop_p=0.1),                   # dx_drop shares lddx; its index uses D
    _c(9, 132, dt, lddy=136, lddres=140, lddx=144),         # the 4-wide form's padding
    _c(9, 132, dt, lddx=140, drop_p=0.1, big=True),
)]
# options
CASES += [c for r, D, dt in ((37, 768, bf), (37, 132, f32)) for c in (
    _c(r, D, dt, dres=False),
    _c(r, D, dt, dbeta=False), _c(r, D, dt, dgamma=False),
    _c(r, D, dt, dbeta=False, accumulate=True), _c(r, D, dt, dgamma=False, accumulate=True),
    _c(r, D, dt, accumulate=True),                          # (overwrite onto NaN is every other case's mode)
    _c(r, D, dt, live=29), _c(r, D, dt, live=29, accumulate=True),
    _c(r, D, dt, live=0),                                   # dgamma = dbeta = 0 exactly, dx untouched
    _c(r, D, dt, live=0, **NOPARAMS),
    _c(r, D, dt, rowmap=True),
    _c(r, D, dt, rowmap=True, live=29, dres=False, drop_p=0.1),       # GPT2.backward's ln_f call
    _c(r, D, dt, rowmap=True, live=29, dres=False, drop_p=0.1, accumulate=True, big=True),
)]

# 13 rows: the row map gathers dy row 0 into no row, so it is NaN here, and ln_bwd8_kernel, which reads row 0 for a
# negative entry and selects afterwards, reads that NaN
CASES += [_c(13, D, dt, rowmap=True) for D in (768, 132) for dt in BOTH]

# Three deferred calls reduced by one icap_ln_param_reduce_batch: unlike widths (the narrower items' blocks return
# early) and unlike block counts (10, 3 and 256); accumulate / overwrite / no dbeta
BATCH_CASES = [_c(37, 768, bf, accumulate=True), _c(9, 132, f32), _c(2057, 64, bf, dbeta=False)]


class Rejected:
    """A call icap_layernorm_bwd must refuse on the host (9 rows). why: the requirement it breaks."""

    def __init__(self, why, D, ldx=None, lddy=None, lddres=None, lddx=None, workspace=True, drop_p=0.0):
        self.why, self.D, self.workspace, self.drop_p = why, D, workspace, drop_p
        self.ldx, self.lddy, self.lddres, self.lddx = ldx or D, lddy or D, lddres or D, lddx or D

    def __repr__(self):
        return self.why.replace(" ", "-")


REJECTED = [
    Rejected("D 6", 6, ldx=8, lddy=8, lddres=8, lddx=8),
    Rejected("D 1028", 1028),
    Rejected("D 1544", 1544),
    Rejected("D 1032 lddx 1036", 1032, lddx=1036),          # wide, but not 8-wide
    Rejected("ldx 770", 768, ldx=770), Rejected("lddy 770", 768, lddy=770),
    Rejected("lddres 770", 768, lddres=770), Rejected("lddx 770", 768, lddx=770),
    Rejected("ldx 134", 132, ldx=134), Rejected("lddy 134", 132, lddy=134),
    Rejected("lddres 134", 132, lddres=134), Rejected("lddx 134", 132, lddx=134),
    Rejected("no workspace", 768, workspace=False),
    Rejected("drop_p 1", 768, drop_p=1.0),
]


def accepted(r):
    """icap_layernorm_bwd's requirements restated (all pointers given, bases aligned)."""
    strides = (r.ldx, r.lddy, r.lddres, r.lddx)
    wide = r.D % 8 == 0 and all(s % 8 == 0 for s in strides)
    return (r.D > 0 and r.D % 4 == 0 and (r.D <= 1024 or (r.D <= 1536 and wide)) and all(s % 4 == 0 for s in strides)
            and r.workspace and 0.0 <= r.drop_p < 1.0)


# ------------------------------------------------------------------------------------------------ reference


def gathered_dy(t, n, dtype=torch.float64):
    """dy' [n, D]: dy through the row map, zero where the map is negative."""
    g = t["gather"]
    dy = t["dy"].to(dtype)[g.clamp_min(0)]
    return torch.where((g >= 0)[:, None], dy, torch.zeros_like(dy))


def formula(x, gamma, mean, rstd, dyp, dres, with_abs=False):
    """The module docstring's formula in the dtype of its arguments: dx, dgamma and dbeta summed over all rows
    given (and, with_abs, the three magnitudes A of the bounds)."""
    xh = (x - mean[:, None]) * rstd[:, None]
    gy = dyp * gamma
    m1, m2 = gy.mean(1, keepdim=True), (gy * xh).mean(1, keepdim=True)
    dx = rstd[:, None] * (gy - m1 - xh * m2)
    if dres is not None:
        dx = dx + dres
    out = dict(dx=dx, dgamma=(dyp * xh).sum(0), dbeta=dyp.sum(0))
    if with_abs:
        a = rstd[:, None] * (gy.abs() + gy.abs().mean(1, keepdim=True) + xh.abs() * (gy * xh).abs().mean(1, keepdim=True))
        out.update(A_dx=a if dres is None else a + dres.abs(), A_dgamma=(dyp * xh).abs().sum(0),
                   A_dbeta=dyp.abs().sum(0))
    return out


@functools.lru_cache(maxsize=None)
def reference(case):
    """fp64 over the live rows: dx [live, D], dgamma, dbeta [D] (with the initial gradient when accumulating),
    dx_drop (or None), and the bounds' magnitudes A_dx [live, D], A_dgamma, A_dbeta [D] (the latter two with
    |initial| added)."""
    t = case.inputs()
    n = case.live
    r = formula(t["x"][:n].double(), t["gamma"].double(), t["mean"][:n].double(), t["rstd"][:n].double(),
                gathered_dy(t, n), None if t["dres"] is None else t["dres"][:n].double(), with_abs=True)
    if case.accumulate:
        for k in ("dgamma", "dbeta"):
            r[k] = r[k] + t[k + "0"].double()
            r["A_" + k] = r["A_" + k] + t[k + "0"].double().abs()
    r["dx_drop"] = r["dx"] * case.keep()[:n] * inv_keep(case.drop_p) if case.drop_p > 0 else None
    return r


def ln_bwd_fp32(case, rounded=True):
    """The same formula evaluated by torch in fp32: dx [live, D] (in the case's dtype when `rounded`), dgamma,
    dbeta fp32 [D]."""
    t = case.inputs()
    n = case.live
    r = formula(t["x"][:n].float(), t["gamma"], t["mean"][:n], t["rstd"][:n], gathered_dy(t, n, f32),
                None if t["dres"] is None else t["dres"][:n].float())
    if case.accumulate:
        r["dgamma"], r["dbeta"] = t["dgamma0"] + r["dgamma"], t["dbeta0"] + r["dbeta"]
    if rounded:
        r["dx"] = r["dx"].to(case.dtype)
    return r


# ------------------------------------------------------------------------------------------------ checks


def _ratio(err, tol):
    """max err / tol; an element whose bound is zero must be exact."""
    if err.numel() == 0:
        return 0.0
    q = torch.where(err == 0, torch.zeros_like(err), err / tol)   # (x / 0 = inf, nan error = nan)
    return math.inf if bool(torch.isnan(q).any()) else q.max().item()


def layout(case, rows_values, fill=SENTINEL):
    """The whole dx (or dx_drop) buffer [rows, lddx] a correct call leaves behind when the buffer held `fill`:
    rows_values [live, D] in the live rows' first D columns, everything else untouched."""
    full = torch.full((case.rows, case.lddx), fill, dtype=rows_values.dtype)
    full[:case.live, :case.D] = rows_values
    return full


def untouched(case, got, fill=SENTINEL):
    """Whether every element of the whole buffer `got` [rows, lddx] outside the live rows' first D columns still
    holds `fill`, and every element inside no longer does (|dx| near 96 is out of the inputs' reach)."""
    got = got.detach().double().cpu()
    assert got.shape == (case.rows, case.lddx)
    stored = torch.zeros(got.shape, dtype=torch.bool)
    stored[:case.live, :case.D] = True
    return bool((got[~stored] == fill).all()) and bool((got[stored] != fill).all())


def dx_ratio(case, got, k=None, r16=None):
    """Worst |got - ref| / bound over the live rows' dx (got: the whole buffer [rows, lddx] or [live, D])."""
    ref = reference(case)
    g = got.detach().double().cpu()[:case.live, :case.D]
    r16 = (2.0 ** -8 if case.dtype == bf else 0.0) if r16 is None else r16
    tol = r16 * ref["dx"].abs() + (K_DX if k is None else k) * U * ref["A_dx"]
    return _ratio((g - ref["dx"]).abs(), tol)


def dx_drop_ratio(case, got):
    """The same for dx_drop = dx * keep / (1 - p): the bound scaled by 1 / (1 - p), K_DX + 2 (the fp32 rounding
    of the scale and of the product); a dropped element has bound zero."""
    ref = reference(case)
    g = got.detach().double().cpu()[:case.live, :case.D]
    keep = case.keep()[:case.live]
    tol = (2.0 ** -8 if case.dtype == bf else 0.0) * ref["dx_drop"].abs() + (
        (K_DX + 2) * U * inv_keep(case.drop_p)) * ref["A_dx"] * keep
    return _ratio((g - ref["dx_drop"]).abs(), tol)


def param_ratios(case, dgamma, dbeta, k=None):
    """(dgamma, dbeta) worst error / bound per column; a gradient that was not asked for (None) gives 0."""
    ref = reference(case)
    out = []
    for name, got in (("dgamma", dgamma), ("dbeta", dbeta)):
        if got is None:
            out.append(0.0)
            continue
        err = (got.detach().double().cpu() - ref[name]).abs()
        out.append(_ratio(err, (K_P if k is None else k) * U * ref["A_" + name]))
    return tuple(out)
