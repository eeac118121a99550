"""fp64 references (CPU tensors), cases and bounds of the loss tail: the final LayerNorm's forward
(icap_layernorm_fwd), the fused cross entropy (icap_cross_entropy) and the AdamW step (icap_adamw_step).
test_loss_refs_cpu.py checks the references and the bounds on their own without a GPU (a plain fp32 evaluation of
each formula must stay inside its bound; a deliberately wrong result must not), test_loss_tail_gpu.py checks the
kernels against them. The "reaches" notes of the case lists are read from the dispatch conditions of
csrc/elementwise.hip icap_cross_entropy and csrc/layernorm.hip icap_layernorm_fwd, not observed.

Every check function returns the worst ratio of error to bound it saw (<= 1 passes), so a test can print it.

Cross entropy, dlogits per element (never a max-norm: with N(0, 3^2) logits at V = 50257 only 0.02 % of the
gradient's elements are above 1e-2 of its maximum):

    |got - ref| <= r16 * |ref| + 2e-5 * max(|ref|, p * sc) + CE_FLOOR

  r16 = 2^-8 for bf16 (half an ulp: the one rounding of the fp32 value), 0 for fp32. The element is
  (expf(x - lse) - onehot) * sc with sc = grad_scale / n_valid and p = softmax. The fast exponential's relative
  error is about |x - lse| * 2^-23 plus an ulp, lse itself is off by a few fp32 ulps of a number near 15 (1e-6),
  together about 5e-6 for |x - lse| <= 30; 2e-5 is four times that. Away from the label |ref| = p * sc and the
  bound is the plain relative one. AT the label the element is (p - 1) * sc: the error of p (2e-5 * p) does not
  shrink with 1 - p, so where p > 1/2 (small V: 3 and 7 classes, where a label often holds most of the mass) the
  cancellation leaves an error of 2e-5 * p * sc, not 2e-5 * (1 - p) * sc; the max() above is that term and is
  the plain relative bound wherever p <= 1/2 (every label of the V >= 1000 cases). Without it torch's own fp32
  evaluation misses the plain bound at the label of the fp32 V = 3 case (p = 0.9937, 1.78 x the bound) and of the
  fp32 V = 7, 300-row case (p = 0.9980, 1.21 x); with it they sit at 0.019 and 0.040. CE_FLOOR = 2^-126, the smallest normal fp32 (an exponential that
  underflows may be flushed). Rows whose one logit is 1e4 above the rest have p = 0 or 1 exactly in both
  precisions.
  Losses (scalar and per row): |got - ref| <= 1e-5 * max(1, |ref|).

LayerNorm forward: y fp32 |d| <= 1e-5 * max|ref|; y bf16 per element |d| <= 2^-8 * |ref| + 1e-5 * max|ref|;
mean |d| <= 64 * 2^-24 * mean_r|x|; rstd relative 128 * 2^-24 (each lane adds at most 48 values, then a 5-step
tree; a plain fp32 evaluation measures about 6e-8 and 1.4e-7).

AdamW: step exact; norm and clip relative 1e-6 (clip exactly 1 where clipping does not apply); lr, step_size,
bc2_sqrt, decay relative 2^-22 (fp64 on the device, rounded once); P and both moments max-abs over max-ref
< 1e-6; the update P_k - P_0 against the reference update < 1e-5 of its max. That last bound decides the inputs:
P is stored in fp32 and rounded twice per step (decay, then the update), 2 * 2^-24 * |p| each step, while the
smallest update it is compared with is the first warmup step's, lr / 3. So 9 steps need
9 * 2^-23 * max|p| <= 1e-5 * lr / 3 in the worst case: the cases use lr = 1e-2 and parameters ~ 0.005 * N(0, 1)
(max|p| about 0.02: 2e-8 against 3e-8).
"""

import functools
import math

import numpy as np
import torch

from dropout_refs import LnCase, randn

bf, f32 = torch.bfloat16, torch.float32
SENTINEL = -96.0        # exact in bf16: output elements a kernel must not touch
STAT_SENTINEL = -7.0    # the same for mean / rstd / per-row losses


def f32r(v):
    """A Python float as the C struct carries it (float)."""
    return float(np.float32(v))


def dt_name(dt):
    return "bf16" if dt == bf else "f32"


# ------------------------------------------------------------------------------------------------ cross entropy

CE_FLOOR = 2.0 ** -126
CE_REL = 2e-5
LOSS_TOL = 1e-5
EQ_VALUE = 1.5          # the all-equal row's logit (exact in bf16): loss = log V
SPIKE = 1e4             # the one large logit of the spike row


class CeCase:
    """rows x V logits with row stride ld. offset: element offset of dlogits (and, in place, of logits) from a
    16-byte aligned base. live: the device row count rows_dev (None: no rows_dev, every row lives)."""

    def __init__(self, name, dtype, V, ld, reaches, rows=24, offset=0, live=None, grad_scale=1.0, dlogits=True):
        self.name, self.dtype, self.V, self.ld, self.reaches, self.rows = name, dtype, V, ld, reaches, rows
        self.offset, self.rows_dev, self.grad_scale, self.dlogits = offset, live, grad_scale, dlogits
        self.live = rows if live is None else live

    def __repr__(self):
        return self.name

    def labels(self):
        """int32 [rows]. Over the live rows: -100 on the first, on the last and on a run of three; then, where V
        has room, label 0, V - 1 (in the V % 8 tail where there is one), 4095 and 4096 (first / second register
        slot of ce_bf16_reg_kernel), 1000 and 1001 (the two halves of one 32-bit pair); the rest random."""
        n, V = self.live, self.V
        y = torch.randint(0, V, (self.rows,), generator=torch.Generator().manual_seed(51), dtype=torch.int32)
        special = [v for v in (0, V - 1, 4095, 4096, 1000, 1001) if 0 <= v < V]
        for i, v in enumerate(special):
            if 1 + i < n - 1:
                y[1 + i] = v
        y[0] = -100
        y[n - 1] = -100
        if n >= 16:
            y[10:13] = -100
        return y

    # rows 7 and 8 carry the two special rows (past the special labels, before the ignored run)
    def inputs(self):
        """logits [rows, ld] in the case's dtype (N(0, 3^2); columns V..ld hold values too: they are never read;
        row 7 all equal, row 8 one logit at 1e4 away from its label; rows past `live` NaN) and labels."""
        rows, V, ld = self.rows, self.V, self.ld
        x = randn((rows, ld), 50, 3.0)
        y = self.labels()
        if self.live > 9:
            x[7, :V] = EQ_VALUE
            if V > 1:
                c = (int(y[8]) + 1 + V // 2) % V
                x[8, c if c != int(y[8]) else (c + 1) % V] = SPIKE
        x[self.live:] = float("nan")
        return dict(logits=x.to(self.dtype), labels=y)


_R, _T = "ce_bf16_reg_kernel<13>", "ce_kernel"
CE_CASES = [
    CeCase("bf16-50257/50304", bf, 50257, 50304, _R),                       # 1-element tail, padding columns
    CeCase("bf16-50264/50264", bf, 50264, 50264, _R),                       # no tail, no padding
    CeCase("bf16-4000/4000-gs.25", bf, 4000, 4000, _R, grad_scale=0.25),    # threads 500.. hold only -inf padding
    CeCase("bf16-53248/53248", bf, 53248, 53248, _R),                       # largest register-form V
    CeCase("bf16-53256/53256", bf, 53256, 53256, _T + "<bf16>"),            # first V past it
    CeCase("bf16-50257/50260", bf, 50257, 50260, _T + "<bf16>"),            # ld % 8 != 0
    CeCase("bf16-50257/50304-off4", bf, 50257, 50304, _T + "<bf16>", offset=4),  # dlogits not 16-byte aligned
    CeCase("bf16-7/8", bf, 7, 8, _R),                                       # V8 == 0: the row in the tail loop
    CeCase("bf16-1/8", bf, 1, 8, _R),                                       # loss 0, gradient 0
    CeCase("f32-50257/50260", f32, 50257, 50260, _T + "<float>"),
    CeCase("f32-1000/1024-gs.25", f32, 1000, 1024, _T + "<float>", grad_scale=0.25),
    CeCase("f32-3/4", f32, 3, 4, _T + "<float>"),                           # V4 == 0
    CeCase("bf16-7/8-300rows", bf, 7, 8, _R, rows=300),                     # ce_reduce_kernel's loop
    CeCase("f32-7/8-300rows", f32, 7, 8, _T + "<float>", rows=300),
    CeCase("bf16-50257/50304-rowsdev17", bf, 50257, 50304, _R, live=17),
    CeCase("f32-1000/1024-rowsdev17", f32, 1000, 1024, _T + "<float>", live=17),
    CeCase("bf16-50257/50304-lossonly", bf, 50257, 50304, _R, dlogits=False),
    CeCase("f32-1000/1024-lossonly", f32, 1000, 1024, _T + "<float>", dlogits=False),
]


@functools.lru_cache(maxsize=None)
def ce_reference(case):
    """fp64 over the live rows: loss (float), loss_rows [live], dlogits [live, ld] (zero for ignored rows and for
    columns V..ld), psc [live, ld] = softmax * sc (the bound's label term), n_valid."""
    t = case.inputs()
    n, V = case.live, case.V
    x = t["logits"][:n, :V].double()
    y = t["labels"][:n].long()
    valid = y >= 0
    nv = int(valid.sum())
    lse = torch.logsumexp(x, 1)
    xy = x.gather(1, y.clamp_min(0)[:, None])[:, 0]
    loss_rows = torch.where(valid, lse - xy, torch.zeros_like(lse))
    p = torch.exp(x - lse[:, None])
    onehot = torch.zeros_like(p)
    onehot[torch.arange(n)[valid], y[valid]] = 1.0
    sc = f32r(case.grad_scale) / nv
    d = torch.zeros((n, case.ld), dtype=torch.float64)
    psc = torch.zeros((n, case.ld), dtype=torch.float64)
    d[:, :V] = (p - onehot) * sc * valid[:, None]
    psc[:, :V] = p * sc * valid[:, None]
    return dict(loss=(loss_rows.sum() / nv).item(), loss_rows=loss_rows, dlogits=d, psc=psc, n_valid=nv)


def ce_fp32(case):
    """(loss, loss_rows, dlogits [live, ld] in the case's dtype): the formula evaluated by torch in fp32."""
    t = case.inputs()
    n, V = case.live, case.V
    x = t["logits"][:n, :V].float()
    y = t["labels"][:n].long()
    valid = y >= 0
    nv = torch.tensor(float(valid.sum()), dtype=f32)
    lse = torch.logsumexp(x, 1)
    xy = x.gather(1, y.clamp_min(0)[:, None])[:, 0]
    loss_rows = torch.where(valid, lse - xy, torch.zeros_like(lse))
    onehot = torch.zeros_like(x)
    onehot[torch.arange(n)[valid], y[valid]] = 1.0
    sc = torch.tensor(case.grad_scale, dtype=f32) / nv
    d = torch.zeros((n, case.ld), dtype=f32)
    d[:, :V] = (torch.exp(x - lse[:, None]) - onehot) * sc * valid[:, None]
    return (loss_rows.double().sum() / nv.double()).float().item(), loss_rows, d.to(case.dtype)


def ce_dlogits_ratio(case, got):
    """Worst |got - ref| / bound over the live rows' dlogits (got: [live, ld], any float dtype)."""
    ref = ce_reference(case)
    d = ref["dlogits"]
    r16 = 2.0 ** -8 if case.dtype == bf else 0.0
    tol = r16 * d.abs() + CE_REL * torch.maximum(d.abs(), ref["psc"]) + CE_FLOOR
    return ((got.detach().double().cpu() - d).abs() / tol).max().item()


def loss_ratio(got, ref):
    """Worst |got - ref| / (1e-5 * max(1, |ref|)) of a loss or a vector of per-row losses."""
    got = torch.as_tensor(got).detach().double().cpu().reshape(-1)
    ref = torch.as_tensor(ref).double().reshape(-1)
    return ((got - ref).abs() / (LOSS_TOL * ref.abs().clamp_min(1.0))).max().item()


def old_ce_check(got, ref):
    """test_kernels_gpu.py test_cross_entropy's measure: max-abs over max-ref."""
    return ((got.double() - ref).abs().max() / ref.abs().max()).item()


# ------------------------------------------------------------------------------------------------ LayerNorm forward

LN_EPS = 1e-5
LN_MEAN_TOL = 64 * 2.0 ** -24
LN_RSTD_TOL = 128 * 2.0 ** -24


class LnFwdCase:
    """x [rows, D] (row stride ldx) -> y (row stride ldy). stats: mean / rstd requested. rowmap: y_rowmap, a
    permutation of the rows with every fourth entry -1 (LnCase.inputs()). live: rows_dev (None: none)."""

    def __init__(self, name, dtype, rows, D, reaches, ldx=None, ldy=None, stats=True, rowmap=False, live=None):
        self.name, self.dtype, self.rows, self.D, self.reaches = name, dtype, rows, D, reaches
        self.ldx, self.ldy = ldx or D, ldy or D
        self.stats, self.rowmap, self.rows_dev = stats, rowmap, live
        self.live = rows if live is None else live

    def __repr__(self):
        return self.name

    def inputs(self):
        """LnCase.inputs() of the same (rows, D): x (rows past `live` NaN), gamma, beta, rowmap (or None)."""
        t = LnCase(self.name, self.dtype, self.rows, self.D, rowmap=self.rowmap).inputs()
        x = t["x"].clone()
        x[self.live:] = float("nan")
        return dict(x=x, gamma=t["gamma"], beta=t["beta"], rowmap=t["rowmap"])


def _chunks(D):
    return 3 if D <= 768 else 4 if D <= 1024 else 5 if D <= 1280 else 6


def _ln(rows, D, dt, **kw):
    wide = D % 8 == 0 and kw.get("ldx", D) % 8 == 0 and kw.get("ldy", D) % 8 == 0
    reaches = f"ln_fwd8_kernel<{dt_name(dt)}, {_chunks(D)}>" if wide else f"ln_fwd_kernel<{dt_name(dt)}>"
    tag = "".join(f"-{k}{v}" for k, v in kw.items())
    return LnFwdCase(f"{rows}x{D}-{dt_name(dt)}{tag}", dt, rows, D, reaches, **kw)


LN8_D = [8, 256, 512, 768, 776, 1024, 1032, 1280, 1288, 1536]   # 776 / 1032 / 1288: first D of the 4 / 5 / 6 chunks
LN4_D = [4, 132, 1020]                                          # 1020: all four float4 groups live
LN_FWD_CASES = [_ln(9, D, dt) for D in LN8_D + LN4_D for dt in (bf, f32)]
LN_FWD_CASES += [c for dt in (bf, f32) for c in (
    _ln(9, 768, dt, ldx=772),                    # 4-wide: stride not a multiple of 8
    _ln(9, 768, dt, ldy=772),                    # x fits the 8-wide form, y does not: the pair falls back
    _ln(9, 768, dt, ldy=776),                    # 8-wide, padding columns must survive
    _ln(9, 132, dt, ldy=140),                    # 4-wide, the same
    _ln(9, 768, dt, stats=False),
    _ln(9, 132, dt, stats=False),
    _ln(4096 * 8 + 9, 64, dt),                   # past the grid cap: ln_fwd8_kernel's row loop runs twice
    _ln(4096 * 4 + 5, 36, dt),                   # ln_fwd_kernel's
)]
LN_FWD_CASES += [_ln(r, D, dt) for r in (1, 7, 8, 37) for D in (768, 132) for dt in (bf, f32)]
LN_FWD_CASES += [c for D, dt in ((768, bf), (132, f32)) for c in (
    _ln(37, D, dt, rowmap=True),
    _ln(37, D, dt, live=29),
    _ln(37, D, dt, rowmap=True, live=29),        # the compact head's combination
)]
# (D, ldx): rejected on the host, nothing is launched
LN_REJECTED = [(6, 8), (1028, 1028), (1544, 1544), (768, 770)]


@functools.lru_cache(maxsize=None)
def ln_fwd_reference(case):
    """fp64 over the live rows: y [live, D], mean, rstd, absx = mean_r |x| [live]."""
    t = case.inputs()
    x = t["x"][:case.live].double()
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / torch.sqrt(var + f32r(LN_EPS))
    y = (x - mean[:, None]) * rstd[:, None] * t["gamma"].double() + t["beta"].double()
    return dict(y=y, mean=mean, rstd=rstd, absx=x.abs().mean(1))


def ln_fwd_fp32(case):
    """(y [live, D] in the case's dtype, mean, rstd): the formula evaluated by torch in fp32."""
    t = case.inputs()
    x = t["x"][:case.live].float()
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / torch.sqrt(var + LN_EPS)
    y = (x - mean[:, None]) * rstd[:, None] * t["gamma"] + t["beta"]
    return y.to(case.dtype), mean, rstd


def ln_dest(case):
    """int64 [live]: the y row of live row r (negative: not stored)."""
    rm = case.inputs()["rowmap"]
    return torch.arange(case.live) if rm is None else rm[:case.live].long()


def ln_layout(case, y_rows):
    """The whole y buffer [rows, ldy] (same dtype as y_rows [live, D]) a correct call leaves behind when the
    buffer was filled with SENTINEL: row r at y row ln_dest(r), everything else untouched."""
    full = torch.full((case.rows, case.ldy), SENTINEL, dtype=y_rows.dtype)
    dest = ln_dest(case)
    full[dest[dest >= 0], :case.D] = y_rows[dest >= 0]
    return full


def ln_y_check(case, got):
    """got: the whole y buffer [rows, ldy] after the call (filled with SENTINEL before). Returns (worst
    |got - ref| / bound over the stored elements, whether every other element still holds SENTINEL)."""
    ref = ln_fwd_reference(case)["y"]
    got = got.detach().double().cpu()
    dest = ln_dest(case)
    stored = torch.zeros((case.rows, case.ldy), dtype=torch.bool)
    stored[dest[dest >= 0], :case.D] = True
    untouched = bool((got[~stored] == SENTINEL).all())
    r = ref[dest >= 0]
    tol = (2.0 ** -8 * r.abs() if case.dtype == bf else 0.0) + 1e-5 * ref.abs().max()
    return ((got[dest[dest >= 0], :case.D] - r).abs() / tol).max().item(), untouched


def ln_stats_ratio(case, mean, rstd):
    """(mean, rstd) worst error over bound, over the live rows."""
    ref = ln_fwd_reference(case)
    n = case.live
    m = (mean[:n].detach().double().cpu() - ref["mean"]).abs() / (LN_MEAN_TOL * ref["absx"])
    r = (rstd[:n].detach().double().cpu() - ref["rstd"]).abs() / (LN_RSTD_TOL * ref["rstd"])
    return m.max().item(), r.max().item()


# ------------------------------------------------------------------------------------------------ AdamW

ADAM_STATE_TOL = 2.0 ** -22
ADAM_FIELDS = ("norm", "clip", "lr", "step_size", "bc2_sqrt", "decay")   # state floats [2] .. [7]


class AdamCase:
    def __init__(self, name, n=4099, steps=3, lr=1e-2, weight_decay=0.01, max_norm=1.0, warmup=0, total=10,
                 gscale=0.05, bf16_out=True, p_only=False):
        self.name, self.n, self.steps, self.lr, self.weight_decay, self.max_norm = name, n, steps, lr, weight_decay, max_norm
        self.warmup, self.total, self.gscale, self.bf16_out, self.p_only = warmup, total, gscale, bf16_out, p_only
        self.betas, self.eps = (0.9, 0.999), 1e-8

    def __repr__(self):
        return self.name

    def inputs(self):
        """p0 [n] ~ 0.005 * N(0, 1) (the module docstring says why), grads: one [n] per step, gscale * N(0, 1)."""
        return (randn((self.n,), 60, 0.005),
                [randn((self.n,), 61 + k, self.gscale) for k in range(self.steps)])

    def kwargs(self):
        return dict(lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=self.weight_decay,
                    max_norm=self.max_norm, num_warmup_steps=self.warmup, num_training_steps=self.total)


# gradient norms at n = 4099: gscale 0.05 -> 3.2 (clipped at max_norm 1), 0.001 -> 0.064 (not clipped)
ADAM_CASES = [
    # lr 0 at step 0, the ramp, the decay, lam == 0 at step 8
    AdamCase("warmup3-total8", steps=9, warmup=3, total=8),
    AdamCase("clip-inactive", gscale=0.001),
    AdamCase("clip-disabled", max_norm=0.0, gscale=1.0),
    AdamCase("no-weight-decay", weight_decay=0.0),
    AdamCase("no-bf16-copy", bf16_out=False),
] + [AdamCase(f"n{n}", n=n) for n in (1, 3, 4, 5)] + [  # tail only (1, 3), one group, group plus tail
    # adam_update_kernel's grid-stride loop runs twice (grid cap 4096 blocks of 256 float4 groups)
    AdamCase("grid-loop", n=4 * 256 * 4096 + 4, steps=1, p_only=True),
]


def schedule_lam(k, warmup, total):
    """HF get_linear_schedule_with_warmup's factor at completed-step count k."""
    if k < warmup:
        return k / max(1, warmup)
    return max(0.0, (total - k) / max(1, total - warmup))


@functools.lru_cache(maxsize=None)
def adamw_reference(case):
    """fp64 restatement of clip_grad_norm_ + AdamW + the linear schedule with warmup, hyper-parameters rounded to
    fp32 first. One dict per step: P, M1, M2 (fp64 [n]) and the documented state fields after that step."""
    p0, grads = case.inputs()
    lr0, b1, b2, eps, wd, mx = (f32r(v) for v in (case.lr, *case.betas, case.eps, case.weight_decay, case.max_norm))
    p, m, v = p0.double().clone(), torch.zeros(case.n, dtype=torch.float64), torch.zeros(case.n, dtype=torch.float64)
    out = []
    for k in range(case.steps):
        g = grads[k].double()
        norm = g.pow(2).sum().sqrt().item()
        clip = min(1.0, mx / (norm + 1e-6)) if mx > 0 else 1.0
        lr = lr0 * schedule_lam(k, case.warmup, case.total)
        t = k + 1
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        g = g * clip
        p = p * (1.0 - lr * wd)
        m = m + (1.0 - b1) * (g - m)
        v = v * b2 + (1.0 - b2) * g * g
        p = p - (lr / bc1) * (m / (v.sqrt() / math.sqrt(bc2) + eps))
        out.append(dict(P=p.clone(), M1=m.clone(), M2=v.clone(), step=t, norm=norm, clip=clip, lr=lr,
                        step_size=lr / bc1, bc2_sqrt=math.sqrt(bc2), decay=1.0 - lr * wd))
    return out


def adamw_fp32(case):
    """The same steps with the element arithmetic in fp32 (the scalars rounded once from fp64, as the device state
    holds them). One dict per step as adamw_reference gives, P / M1 / M2 in fp32."""
    p0, grads = case.inputs()
    ref = adamw_reference(case)
    b1, b2, eps = (torch.tensor(v, dtype=f32) for v in (*case.betas, case.eps))
    p, m, v = p0.clone(), torch.zeros(case.n), torch.zeros(case.n)
    out = []
    for k in range(case.steps):
        s = {f: torch.tensor(ref[k][f], dtype=f32) for f in ADAM_FIELDS}
        s["norm"] = grads[k].pow(2).sum().sqrt()
        if f32r(case.max_norm) > 0:
            s["clip"] = torch.clamp(torch.tensor(case.max_norm, dtype=f32) / (s["norm"] + 1e-6), max=1.0)
        g = grads[k] * s["clip"]
        p = p * s["decay"]
        m = m + (1 - b1) * (g - m)
        v = v * b2 + (1 - b2) * (g * g)
        p = p + (-s["step_size"]) * (m / (v.sqrt() / s["bc2_sqrt"] + eps))
        out.append(dict(P=p.clone(), M1=m.clone(), M2=v.clone(), step=k + 1, **{f: s[f].item() for f in ADAM_FIELDS}))
    return out


def _maxrel(a, b, scale=None):
    a, b = a.detach().double().cpu(), b.double()
    return ((a - b).abs().max() / (b if scale is None else scale).abs().max().clamp_min(1e-300)).item()


def adam_step_ratios(case, k, got):
    """got: dict with P, M1, M2 (tensors) and the state fields after step k (0-based). Returns {name: error over
    bound}; `step` and an inapplicable clip are compared exactly (ratio 0 or inf)."""
    p0, _ = case.inputs()
    ref = adamw_reference(case)[k]
    r = {"P": _maxrel(got["P"], ref["P"]) / 1e-6}
    if case.p_only:
        return r
    r["M1"] = _maxrel(got["M1"], ref["M1"]) / 1e-6
    r["M2"] = _maxrel(got["M2"], ref["M2"]) / 1e-6
    upd = ref["P"] - p0.double()
    if upd.abs().max() > 0:
        r["update"] = _maxrel(got["P"].detach().double().cpu() - p0.double(), upd) / 1e-5
    tail = case.n - case.n % 4
    if case.n % 4 and tail:   # the scalar tail's error on its own, over the whole tensor's max (n < 4 is all tail)
        for f in ("P", "M1", "M2"):
            r[f + "-tail"] = _maxrel(got[f][tail:], ref[f][tail:], ref[f]) / 1e-6
    r["step"] = 0.0 if int(got["step"]) == ref["step"] else math.inf
    for f, tol in (("norm", 1e-6), ("clip", 1e-6), ("lr", ADAM_STATE_TOL), ("step_size", ADAM_STATE_TOL),
                   ("bc2_sqrt", ADAM_STATE_TOL), ("decay", ADAM_STATE_TOL)):
        d = abs(float(got[f]) - ref[f])
        r[f] = 0.0 if d == 0 else d / (tol * abs(ref[f])) if ref[f] != 0 else math.inf
    if ref["clip"] == 1.0 and float(got["clip"]) != 1.0:
        r["clip"] = math.inf
    return r
