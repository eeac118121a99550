"""fp64 references (CPU tensors), inputs, per-element bounds and the case list of the LayerNorm forms of icap_gemm on
every kernel family: the statistics producer (ln_stats_out, kind ACT_LNS), the consumer (ln_stats_in + ln_wsum, kind
ACT_LNF), the decode fold (ln_wsum alone, skinny kernel), the fused LayerNorm (ln_gamma / ln_beta, skinny kernel) and
a producer launch chained into a consumer launch. test_gemm_ln_refs_cpu.py checks all of it without a GPU;
test_gemm_ln_gpu.py runs every case on the device. Activations, the sentinel, C_ACC / ACT_REL / ACT_ABS / R16, the
kernel-name convention and the planted producer rows are gemm_epi_refs.py's; what is restated here is only the tail
of its bound (bounds()'s lines after dz), which that module does not expose as a function of z and dz.

References (include/icap.h icap_gemm_args ln_gamma / ln_wsum / ln_stats_*, fp64, from exactly the operands the launch
is given: B, ln_wsum, bias are whatever stored values the case hands over, the host-side fold is no part of it):

  producer  C as gemm_epi_refs (alpha acc + bias + resid, alpha = 0.5, dropout off) against that module's bound; then
            per row and 32-column group of the C the launch STORED, mean and sum (x - mean)^2 in fp64. C is checked
            against its own reference and the statistics against the stored C, so the two budgets stay apart. Where
            the fp64 C lies within the accumulation error of a bf16 rounding boundary the stored value may be either
            neighbour (inside C's bound): over the 18 producer cases the plain fp32 evaluation stores the other
            neighbour in none of the elements of the exact rows 0-23 and in 90 of the 2.18 M others (flips(), printed).
  consumer  from the given fp32 statistics st[m, g] = (mean_g, M2_g), G = K / 32: mean = sum_g mean_g / G,
            M2 = sum_g M2_g + 32 sum_g (mean_g - mean)^2, rstd = 1 / sqrt(M2 / K + eps);
            z = rstd (A . B^T - mean wsum) + bias; aux = z (tanh: act(z)); C = act(z) + resid.
            ln_mean_out / ln_rstd_out against mean / rstd.
  fold      the same z with mean and the population variance of the stored A row (fp64 over its K values).
  fused     a = round_in(((x - mean) rstd) gamma + beta) (the input dtype's rounding; none for fp32), then
            z = a . B^T + bias and the same tail.
  chained   a real producer launch's C and statistics are the consumer's A and ln_stats_in; the end result against
            fp64 LN(stored C) . B^T + bias with the EXACT statistics of the stored C. The bound is the consumer's bound
            with the producer's statistics bounds added to its mean and M2 errors (the sum of the two).

Bounds, per element; every check returns the worst ratio of error to bound (<= 1 passes): no max-norm, no excluded
element, no retry. U = 2^-24 (one fp32 rounding); every count below is multiplied by MARGIN = 4, as in loss_refs.py /
gemm_epi_refs.py, except dacc = C_ACC |A| . |B|^T, which is that module's (already generous) accumulation constant.

  producer statistics (gemm_tile.h store_row LNX == 1, gemm8p.hip l.381-401: each of 4 lanes adds its EW <= 8 stored
  values in turn, two cross-lane adds, * 1/32 exact; then d = x - mean, d * d, the same sum):
    dmean_g = 10 U sum|x| / 32                (a value passes through <= EW + 2 = 10 adds)
    dM2_g   = 13 U M2 + 2 sum|x - mean| dmean_g + 32 dmean_g^2
              (subtract, square, 10 adds + one spare; the mean's own rounding moves every d by dmean_g)
    Groups of 32 equal values give mean = x and M2 = 0 with no error at all; the bound does not need that.
  consumer row statistics (gemm_tile.h l.267-312, gemm8p.hip l.146-181: a thread adds its G / 2 group means in turn, one
  pair shuffle, one division; second pass d = mean_g - mean, 32 d d, + M2_g, G / 2 + 1 adds, one shuffle):
    dmean = (G / 2 + 2) U sum|mean_g| / G
    e_g   = dmean + U |mean_g - mean|  [+ the producer's dmean_g when chained]
    dM2   = (G + 8) U M2 + 32 sum_g (2 |mean_g - mean| e_g + e_g^2)  [+ sum_g dM2_g when chained]
    dvar  = dM2 / K + 2 U (M2 / K + eps)       (the division and the add of eps)
    drstd / rstd = (1 - dvar / var)^(-1/2) - 1 + 4 U     (sqrtf and the reciprocal division: one ulp = 2 U each)
  ln_mean_out within dmean, ln_rstd_out within rstd drstd / rstd.
  pre-activation, t = rstd (acc - mean wsum):
    dz = rstd (dacc + 2^-23 (|acc| + |mean wsum|) + dmean |wsum|) + |t| (drstd / rstd + U) + U (|t| + |bias|)
  The first part is ABSOLUTE in rstd: the product mean wsum and the subtraction round once each at the size of their
  operands, not of the difference. It is never relative to |acc - mean wsum|: on a constant row that difference is 0
  (up to dacc and wsum's own fp32 rounding) and rstd is 1 / sqrt(eps) = 316. The middle part is rstd's relative error
  on what it scales; the last the fma with bias.
  fold / fused row statistics (gemm.hip l.128-281), by the path the launch takes (Case.frag). bf16 rows that fit the
  fragment registers take ONE pass over d = x - x0, x0 the row's first element: a thread adds its K / 32 values of d
  and of d d in turn, 2 cross-lane adds, 8 wave partials, one division, n = K / 32 + 11; mean = x0 + E d, var = E d^2 -
  (E d)^2, whose two parts cancel:
    dmean = n U sum|x - x0| / K + U |mean|        dvar = (n + 3) U (var + 2 (mean - x0)^2) + 2 U (var + eps)
  Every other launch (fp32 rows; bf16 with K > 1536) takes two passes, 16 threads per row, K / 16 adds and 4 shuffles
  and one division each, n = K / 16 + 5:
    dmean = n U sum|x| / K      dvar = (n + 2) U var + 2 dmean sum|x - mean| / K + dmean^2 + 2 U (var + eps)
  drstd / rstd as above; dz as the consumer's.
  fused: da = |rstd gamma| (dmean + U |x - mean|) + |(x - mean) rstd gamma| (drstd / rstd + 2 U) + U |a| per element of a
  (gemm.hip ln_chunk: subtract, two products, one add). fp32 inputs: dacc = da . |B|^T + C_ACC |a| . |B|^T. bf16 inputs:
  the device rounds ITS a to bf16; that equals the reference's round(a) unless the fp64 a lies within da of a rounding
  boundary, so the bound carries flip_k |b_k| for those k only, flip_k = |round(a +- da) - round(a)| (one bf16 ulp of
  a_k), never 2^-8 sum |a| |b| wholesale: dacc = flip . |B|^T + C_ACC |round a| . |B|^T. Share of such k
  (boundary_share(), printed): 1.4-1.6 % of the elements of a on the random rows at K = 200 and 4.8 % at K = 1600 (the
  two-pass loop's 105 adds widen dmean); 4.6-4.9 % and 10.4 % over all rows, because on the planted constant, offset-300
  and tiny-variance rows rstd dmean is of the size of a bf16 ulp of a and most of their k count.
  tail (gemm_epi_refs bounds(), restated): C within r16 |ref| + L_act dz + act_term(z) + 2^-23 (|act z| + |resid|),
  aux within r16 |aux| + dz (tanh: L dz + act_term).

Inputs. Consumer / fold / fused A: random rows N(0.5, 2^2) with column 7 offset by +30 (the residual stream's shape),
rounded to the input dtype, and planted rows 0-10 for which the answer is known and which tell right from wrong:
  0, 1  constant (1.5; 300): M2 = 0, rstd = 1 / sqrt(eps), z = bias up to the absolute term
  2     300 + 2 {-1, 0, 1}: mean ~ 300, spread ~ 1.6 (bf16 is 2 apart there); 3: 300 with every 32nd element 302
        (spread 0.35): a one-pass E x^2 - mean^2 fails, and so does a combine that squares the group means
  4, 5  equal spread (+-0.5) within every group, group means 8 (g % 5 - 2) / -16 (g % 2): the between-group term is
        all but 0.25 of the variance
  6     equal group means (0), spreads 2^(g % 4 - 2): the converse
  7, 8  0.25 +- 2^-9 and +- 2^-9: variance 3.8e-6 < eps, where eps misplaced or missing shows
  9     a random row whose FIRST element is offset by +30 (the one-pass fold form's x0)
  10    300 + 0.01 N(0, 1): for fp32 inputs a spread 3e4 below the offset, where an fp32 E x^2 - mean^2 is noise (in
        bf16 it rounds to a third constant row)
B ~ N(0, 2.4^2 / K), bias ~ N(0, 0.9^2), wsum = fp32(sum_k B in fp64), gamma = 1 + 0.2 N, beta = 0.1 N, eps = 1e-5,
ln_stats_in = fp32 of the fp64 group statistics of the stored A. Producer: gemm_epi_refs.inputs (rows 0-15 unit
vectors: stored values known exactly) with rows 16-23 of A zeroed and bias 0 on columns 0-63, so there C = resid
exactly, and resid planted: 16 all 3.140625 (M2 = 0), 17 groups of 31 equal values and one outlier (100; -64),
18 300 + 2 {-1, 0, 1}, 19 one group of 32 x 300 and one with a single 302.

Cases (CASES; each names the instantiation it must plan to and launch). The LayerNorm kinds are not typed in: every
family below asks the host-only planner for the producer and for the consumer with no activation, gelu_new, quick_gelu
and tanh at its shape, and keeps each request that plans to a further LN kind of the family's own kernel (on variants
12 / 13 an activated request plans to the dispatching kind; elsewhere tanh has no form and quick_gelu on variant 0 moves
to variant 4). test_gemm_ln_refs_cpu.test_kinds_match_the_table counts the result against tests/golden/gemm_kernel_forms.json
(the table of forms as built): 44 LN instantiations = 13 producer + 22 consumer kinds + 3 of variant 5 (planned by the
diagnostic build only, left out as before) + 6 8-phase forms with an fp32 C (instantiated, but gemm_validate requires
a bf16 C for ln_stats_*: unreachable). Producers: variants 0, 4, 12, 13, 22, 24, 25, 26, 27, 28, 32, g8p 128 / 256.
Consumers: alone on 0, 4, 12, 13, 22, 26, 28, g8p 128 / 256; + gelu_new on 0, 4, 22, 26, 28, g8p 128 / 256; + quick_gelu
on 4, 22, 26, 28; dispatching on 12, 13. Shapes are the smallest at which each family is eligible, with a partial row
tile, a partial column tile and (consumer) at least two column tiles: producer 300 x 288 x 200 (N % 32 == 0, 4.5 / 2.25
/ 1.125 tiles of 64 / 128 / 256 columns), 100 x 160 x 200 on variant 4, 130 x 8160 x 64 on 13, K = 1096 on 0 / 25;
consumer 300 x 264 x K (100 x 264 on variant 4, 200 x 264 on 0, 130 x 8136 on 13) with every kind at K = 384 (12 groups:
an odd number of 16-byte loads per thread; variant 0 plans only past 16 K stages: K = 1280) and the activation-free kind
also at K = 128 (one load per thread) and K = 1280 (the LNQ = 10 limit) where the family plans there. Skinny kernel:
fold and fused, bf16 / bf16, bf16 / fp32 and fp32 / fp32, with and without gelu_new at 100 x 130 x 200 (the one-pass
fragment statistics for bf16), and bf16 at K = 1600 (12 k-steps in flight: the two-pass loop). One chained case per
consumer family (producer N = consumer K = 384). Layout cases on variant 4 and the split-role variant 26, producer and
gelu_new consumer: m_dev = M - 3 with every operand in a padded view (ld % 8 == 0), and m_dev = 37 (inside the first
row tile) with ld = N + 1; ln_stats_out / ln_mean_out / ln_rstd_out are NaN-filled with guard elements around them and
must keep every NaN outside the live rows; ln_stats_in, ln_wsum, bias, A, B, resid must be unmodified. No case has a
device row count of 0 (gemm_tile.h returns at m0 >= Mv before the statistics; gemm8p.hip returns at bid >= nwg = 0:
both read as safe, neither is exercised). In-launch split: the planner gives an LN kind one only past 24 K stages
(gemm_plan.cpp wanted_splits), which the consumer's K <= 1280 never reaches; the producer gets it on variant 0 at
200 x 160 x 1544 (case family v0_split, asserted with icap_gemm_plan_info).

Worst ratios of a plain fp32 torch evaluation on the CPU (test_plain_fp32_inside_bounds, all 80 cases; a bf16 store's
rounding alone reaches the bound of C / aux, so the arithmetic's own figures are the statistics and the fp32-C cases):
    producer  C 0.996  mean_g 0.012  M2_g 0.053
    consumer  C 0.988  aux 0.987  ln_mean_out 0.061  ln_rstd_out 0.058
    chained   C 0.984  aux 0.984  ln_mean_out 0.043  ln_rstd_out 0.019
    fold      bf16 / bf16 C 0.960 aux 0.965;  bf16 / fp32 C 0.020 aux 0.021;  fp32 / fp32 C 0.080 aux 0.081
    fused     bf16 / bf16 C 0.963 aux 0.974;  bf16 / fp32 C 0.537 aux 0.537 (one a on the other side of a boundary);
              fp32 / fp32 C 0.030 aux 0.028
Each of the 17 wrong evaluations of test_gemm_ln_refs_cpu.APPLIES exceeds the bound in every case it applies to.

MEASURED on an MI355X (test_gemm_ln_gpu.py, every element of every case; the named kernel launched, sentinels, NaN
guards, dead rows and read-only operands intact in all 80 cases (89 launches); nothing was found):
    producer (13 kinds + the in-launch split + 4 layouts)   C 0.996 (0.988 split)   mean_g <= 0.010   M2_g <= 0.032
      mean_g 0.000 / M2_g 0.025-0.026 at K = 200 on every family (v4 v12 v22 v24 v26 v27 v28 v32 g8p128 g8p256: the
      same stored C, so the same statistics), 0.008 / 0.032 at K = 1096 (v0, v25), 0.010 / 0.032 on v13
    consumer  family   C      aux    ln_mean_out  ln_rstd_out |  chained  C      aux    ln_mean_out  ln_rstd_out
              v0       0.960  0.958  0.024        0.022       |           0.954  0.957  0.024        0.011
              v4       0.972  0.981  0.045        0.042       |           0.981  0.970  0.029        0.018
              v13      0.988  0.987  0.061        0.042       |           0.986  0.984  0.021        0.016
              v12 v22 v26 v28 g8p128 g8p256 (one shape, equal figures)
                       0.981  0.986  0.050        0.043       |           0.974  0.975  0.006        0.017
      (C / aux are bf16 stores: their rounding alone reaches 1; the row statistics are the arithmetic's own figure)
    fold      bf16 / bf16 C 0.960 aux 0.965 (K = 1600: 0.932 / 0.937);  bf16 / fp32 C 0.009 aux 0.008;
              fp32 / fp32 C 0.030 aux 0.030
    fused     bf16 / bf16 C 0.963 aux 0.974;  bf16 / fp32 C 0.537 aux 0.537 (K = 1600: 0.162; the same elements as
              the plain fp32 evaluation: an a_k on the other side of a bf16 boundary);  fp32 / fp32 C 0.010 aux 0.011
"""

import copy
import functools
import math
import re

import torch

import gemm_epi_refs as R
from gemm_epi_refs import ACT_ABS, ACT_REL, C_ACC, R16, SENTINEL, act_ref, bf, f32, f64, ratio  # noqa: F401
from gemm_plan_cases import gemm_args, plan
from icap import _lib as L

EPS = 1e-5
U = 2.0 ** -24
MARGIN = 4.0
LNS, LNF = 256, 512
_GN, _QG, _TANH = R.ACTS["gelu_new"], R.ACTS["quick_gelu"], R.ACTS["tanh"]
NPLANT = 11


# ------------------------------------------------------------------------------------------------ inputs

def _plant(A, K, g):
    k = torch.arange(K)
    grp, s = k // 32, (1 - 2 * (k % 2)).double()
    A[0] = 1.5
    A[1] = 300.0
    A[2] = 300.0 + 2.0 * torch.randint(-1, 2, (K,), generator=g).double()
    A[3] = 300.0
    A[3, k % 32 == 5] = 302.0
    A[4] = 8.0 * (grp % 5 - 2) + 0.5 * s
    A[5] = -16.0 * (grp % 2) + 0.5 * s
    A[6] = s * 2.0 ** (grp % 4 - 2).double()
    A[7] = 0.25 + s * 2.0 ** -9
    A[8] = s * 2.0 ** -9
    A[9, 0] += 30.0
    A[10] = 300.0 + 0.01 * torch.randn(K, generator=g, dtype=f64)


def group_stats(x):
    """fp64 (mean, M2) per row and 32-column group of x [M, N], N % 32 == 0 -> [M, N / 32, 2]."""
    M, N = x.shape
    g = x.double().reshape(M, N // 32, 32)
    mean = g.mean(-1)
    return torch.stack([mean, ((g - mean[..., None]) ** 2).sum(-1)], -1)


@functools.lru_cache(maxsize=None)
def ln_inputs(in_dt, c_dt, M, N, K):
    """Operands of the consumer / fold / fused forms of one shape (stored dtypes) and their fp64 products."""
    g = torch.Generator().manual_seed(7000 + 1000 * M + 10 * N + K + (3 if in_dt == bf else 0) + (5 if c_dt == bf else 0))
    A = torch.randn((M, K), generator=g, dtype=f64) * 2 + 0.5
    A[:, 7] += 30.0
    _plant(A, K, g)
    x = R.Inputs()
    x.in_dt, x.c_dt, x.M, x.N, x.K = in_dt, c_dt, M, N, K
    x.A = A.to(in_dt)
    if in_dt == bf:
        assert torch.equal(x.A[:9].double(), A[:9])  # the planted rows are bf16-exact
    x.B = (torch.randn((N, K), generator=g, dtype=f64) * (2.4 / math.sqrt(K))).to(in_dt)
    x.bias = (torch.randn(N, generator=g, dtype=f64) * 0.9).to(f32)
    x.wsum = x.B.double().sum(-1).to(f32)
    x.gamma = (1 + 0.2 * torch.randn(K, generator=g, dtype=f64)).to(f32)
    x.beta = (0.1 * torch.randn(K, generator=g, dtype=f64)).to(f32)
    x.resid = torch.randn((M, N), generator=g, dtype=f64).to(c_dt)
    x.stats = x.stats_given = group_stats(x.A).to(f32) if K % 32 == 0 else None
    x.dmg = x.dm2g = None
    _products(x)
    return x


def _products(x):
    x.acc = x.A.double() @ x.B.double().t()
    x.absacc = x.A.double().abs() @ x.B.double().abs().t()


@functools.lru_cache(maxsize=None)
def prod_inputs(M, N, K):
    """gemm_epi_refs.inputs(bf16, bf16) with rows 16-23 planted through resid (module docstring)."""
    x = copy.copy(R.inputs(bf, bf, M, N, K))
    g = torch.Generator().manual_seed(M + N + K)
    A, bias, resid = x.A.clone(), x.bias.clone(), x.resid.clone()
    A[16:24] = 0
    bias[:64] = 0
    r = resid[16:24, :64].double()
    r[0] = 3.140625
    r[1, :32], r[1, 13] = 1.0, 100.0
    r[1, 32:], r[1, 63] = -0.5, -64.0
    r[2] = 300.0 + 2.0 * torch.randint(-1, 2, (64,), generator=g).double()
    r[3], r[3, 40] = 300.0, 302.0
    resid[16:24, :64] = r.to(bf)
    assert torch.equal(resid[16:20, :64].double(), r[:4])
    x.A, x.bias, x.resid = A, bias, resid
    _products(x)
    x.absacc[:R.P] = 0
    assert torch.equal(x.acc[:R.P], x.B[:, :R.P].double().t()) and not x.acc[16:24].any()
    return x


def chain_inputs(c, stored_c, stats):
    """The chained consumer's operands: A = the producer's stored C [M, K2] (CPU, bf16) and ln_stats_in = the
    statistics it wrote (fp32); the reference takes the EXACT statistics of the stored C and the budget the
    producer's statistics bounds; B / wsum / bias / resid by seed."""
    x = copy.copy(ln_inputs(bf, bf, c.M, c.N, c.K))
    x.A, x.stats_given = stored_c.clone(), stats.clone()
    x.stats, x.dmg, x.dm2g = producer_stat_bounds(x.A)
    _products(x)
    return x


# ------------------------------------------------------------------------------------------------ families + cases

_TILE, _ONE = dict(tile_only=True, split_k=1), dict(split_k=1)
_PR, _PL = (300, 288, 200), (300, 288, 1096)


def _cons(M, N, *ks):
    return {k: (M, N, k) for k in ks}


# family -> (ops.gemm keywords, variant or "g8p", producer shape, {K: consumer shape}); the main K is the first
FAMILIES = {
    "v4": (_TILE, 4, (100, 160, 200), _cons(100, 264, 384, 128)),
    "v0": (_TILE, 0, _PL, _cons(200, 264, 1280)),
    "v12": (_TILE, 12, _PR, _cons(300, 264, 384, 128)),
    "v13": (_TILE, 13, (130, 8160, 64), _cons(130, 8136, 384, 128)),
    "v22": (dict(_ONE, r256=True), 22, _PR, _cons(300, 264, 384, 128, 1280)),
    "v24": (dict(_ONE, w192=True), 24, _PR, {}),
    "v25": (dict(_ONE, w192=True), 25, _PL, {}),
    "v26": (dict(_ONE, roles=256), 26, _PR, _cons(300, 264, 384, 128, 1280)),
    "v27": (dict(_ONE, roles=96), 27, _PR, {}),
    "v28": (dict(_ONE, roles=192), 28, _PR, _cons(300, 264, 384, 128, 1280)),
    "v32": (dict(_ONE, roles=160), 32, _PR, {}),
    "g8p128": (dict(_ONE, g8p=128), "g8p", _PR, _cons(300, 264, 384, 128, 1280)),
    "g8p256": (dict(_ONE, g8p=256), "g8p", _PR, _cons(300, 264, 384, 128, 1280)),
    "v0_split": (dict(), 0, (200, 160, 1544), {}),
    "skinny": (dict(), "skinny", None, {}),
}


class Case:
    """One launch (chain: two). Carries the attributes gemm_epi_refs.bounds reads, so the producer's C goes through
    that function unchanged."""
    dact, beta, trans = 0, 0.0, False

    def __init__(self, form, family, shape, act=0, in_dt=bf, c_dt=bf, live=None, layout=R.PLAIN, kind=None):
        self.form, self.family, self.act, self.in_dt, self.c_dt, self.layout = form, family, act, in_dt, c_dt, layout
        self.kw, self.named = FAMILIES[family][:2]
        self.M, self.N, self.K = shape
        self.live = self.M if live is None else live
        self.m_dev = live is not None
        self.alpha = R.ALPHA if form == "producer" else 1.0
        self.bias = self.resid = True
        self.aux = form != "producer"
        self.rows_out = form in ("consumer", "chain")
        self.kind = kind  # the ACT template integer of a tile / 8-phase kernel
        self.name = (f"{family}-{form}" + (f"-{R.ACT_NAME[act]}" if act else "") + f"-{self.M}x{self.N}x{self.K}" +
                     (f"-{R.dt_name(in_dt)}-{R.dt_name(c_dt)}" if family == "skinny" else "") +
                     (f"-live{live}" if self.m_dev else "") + (f"-{layout.name}" if layout is not R.PLAIN else ""))

    def __repr__(self):
        return self.name

    def kernel(self):
        if self.named == "skinny":  # one 16-column slab per block; k-steps in flight: 6 (fp32), 3 / 12 (bf16, K = 200 / 1600)
            sku = 6 if self.in_dt == f32 else 3 if self.K <= 768 else 12
            return f"icap::gemm_skinny_kernel<{R._ctype(self.in_dt)}, {R._ctype(self.c_dt)}, 1, 2, {sku}>"
        if self.named == "g8p":
            return f"icap::gemm8p_kernel<unsigned short, {self.kw['g8p']}, {self.kind}>"
        return R.tile_name(self.named, bf, bf, self.kind)

    @property
    def frag(self):
        """Skinny kernel: the row statistics come from the fragments in one pass (gemm.hip LN_FRAG: bf16, at most 6
        k-steps in flight per wave and all of K in them; one 16-column slab per block: K <= 8 * 6 * 32)."""
        return self.in_dt == bf and self.K <= 1536

    def inputs(self):
        if self.form == "producer":
            return prod_inputs(self.M, self.N, self.K)
        return ln_inputs(self.in_dt, self.c_dt, self.M, self.N, self.K)

    def producer(self):
        """The chain's first launch: same family, N = this case's K."""
        return Case("producer", self.family, (self.M, self.K, 200), kind=LNS)

    def lds(self):
        lay, N = self.layout, self.N
        return lay.ldc or N, lay.ldaux or N, lay.ldr or N, lay.ldd or N


def plan_args(c):
    """icap_gemm_args of the case with fake pointers (the planner reads sizes, strides and alignment only)."""
    ldc, ldaux, ldr, _ = c.lds()
    off = c.layout.off * (2 if c.c_dt == bf else 4)
    ln = {"producer": "stats_out", "consumer": "stats_in", "chain": "stats_in", "fold": "wsum", "fused": "gamma"}[c.form]
    a = gemm_args(c.M, c.N, c.K, in_dtype=L.BF16 if c.in_dt == bf else L.F32, c_dtype=L.BF16 if c.c_dt == bf else L.F32,
                  act=c.act, alpha=c.alpha, path=R.path_of(c.kw), split_k=c.kw.get("split_k", 0), scratch="ws+tickets",
                  m_dev=c.m_dev, ln=ln)
    if c.m_dev:
        a.m_hint = c.live
    a.C, a.ldc, a.bias = (1 << 20) + off, ldc, 1 << 23
    a.resid, a.ldr = (1 << 29) + off, ldr
    if c.aux:
        a.aux, a.ldaux = (1 << 25) + off, ldaux
    if c.rows_out:
        a.ln_mean_out, a.ln_rstd_out = 1 << 30, 1 << 31
    return a


def _kind_of(name):
    return int(re.search(r"(\d+)(?:, true)?>$", name).group(1))


def _planned_kinds(lib):
    """[(family, form, act, kind)]: what the planner gives each family's own kernel for the producer and for the
    consumer without an activation, with gelu_new, quick_gelu and tanh (the dispatching kind)."""
    out = []
    for fam, (kw, named, pshape, cshapes) in FAMILIES.items():
        if pshape is None or fam == "v0_split":
            continue
        reqs = [("producer", pshape, 0)] + [("consumer", next(iter(cshapes.values())), a) for a in (0, _GN, _QG, _TANH)
                                            if cshapes]
        for form, shape, act in reqs:
            c = Case(form, fam, shape, act=act, kind=0)
            name = plan(lib, plan_args(c))[0]
            if not name.startswith("icap::gemm"):
                continue  # no LayerNorm form of this kernel for the request
            c.kind = _kind_of(name)
            if c.kind >= LNS and name == c.kernel() and (fam, c.kind) not in [(f, k) for f, _, _, k in out]:
                out.append((fam, form, act, c.kind))
    return out


def _cases():
    lib = L.load()
    out = []
    kinds = _planned_kinds(lib)
    for fam, form, act, kind in kinds:  # every LayerNorm kind of the table, at the family's main shape
        _, _, pshape, cshapes = FAMILIES[fam]
        out.append(Case(form, fam, pshape if form == "producer" else next(iter(cshapes.values())), act=act, kind=kind))
    for fam, (_, _, _, cshapes) in FAMILIES.items():  # the activation-free consumer at the other K; one chain each
        for shape in list(cshapes.values())[1:]:
            out.append(Case("consumer", fam, shape, kind=LNF))
        if cshapes:
            out.append(Case("chain", fam, next(iter(cshapes.values())), kind=LNF))
    out.append(Case("producer", "v0_split", FAMILIES["v0_split"][2], kind=LNS))
    for in_dt, c_dt in ((bf, bf), (bf, f32), (f32, f32)):
        for form in ("fold", "fused"):
            for act in (0, _GN):
                out.append(Case(form, "skinny", (100, 130, 200), act=act, in_dt=in_dt, c_dt=c_dt))
    out.append(Case("fold", "skinny", (100, 130, 1600)))
    out.append(Case("fused", "skinny", (100, 130, 1600), c_dt=f32))
    for fam in ("v4", "v26"):  # layouts: m_dev = M - 3 in padded views, m_dev inside the first row tile with ld = N + 1
        _, _, pshape, cshapes = FAMILIES[fam]
        cshape = next(iter(cshapes.values()))
        for shape, form, act, kind in ((pshape, "producer", 0, LNS), (cshape, "consumer", _GN, LNF + R.ACT_FWD + _GN)):
            wide, odd = R.layouts(shape[1])[:2]
            out.append(Case(form, fam, shape, act=act, kind=kind, live=shape[0] - 3, layout=wide))
            out.append(Case(form, fam, shape, act=act, kind=kind, live=37, layout=odd))
    names = [c.name for c in out]
    assert len(set(names)) == len(names), names
    return out, kinds


CASES, KINDS = _cases()


# ------------------------------------------------------------------------------------------------ evaluation

def combine(st, dt, wrong=None):
    """Row (mean, M2) from the group statistics st [M, G, 2], evaluated in dt."""
    mg, m2g = st[..., 0].to(dt), st[..., 1].to(dt)
    G = mg.shape[1]
    n = {"n31": 31.0, "n33": 33.0}.get(wrong, 32.0)
    if wrong == "half_groups":  # the pair shuffle lost: one thread's half of the groups stands for the row
        mg, m2g = mg[:, :G // 2], m2g[:, :G // 2]
    mean = mg[:, :G // 2].mean(-1) if wrong == "half_mean" else mg.mean(-1)
    if wrong == "onepass":
        M2 = m2g.sum(-1) + n * (mg * mg).sum(-1) - n * G * mean * mean
    elif wrong == "no_between":
        M2 = m2g.sum(-1)
    else:
        M2 = m2g.sum(-1) + n * ((mg - mean[:, None]) ** 2).sum(-1)
    return mean, (2 * M2 if wrong == "half_groups" else M2)


def row_stats(A, dt, wrong=None):
    """Row (mean, M2) of the stored A, evaluated in dt (the fold / fused forms)."""
    x = A.to(dt)
    mean = x.mean(-1)
    if wrong == "onepass":
        return mean, ((x * x).mean(-1) - mean * mean).clamp(min=0) * x.shape[1]
    return mean, ((x - mean[:, None]) ** 2).sum(-1)


def rstd_of(M2, K, eps, wrong=None):
    var = M2 / (K - 1 if wrong == "k_minus_1" else K)
    if wrong == "eps_outside":
        return 1 / (var.sqrt() + eps)
    return 1 / (var if wrong == "no_eps" else var + eps).sqrt()


def _tail(c, x, z, dt, wrong=None):
    """(C, aux) before the store's rounding from the pre-activation z (gemm_epi_refs.evaluate's forward tail)."""
    y = z if wrong == "act_first" else act_ref(c.act, z)
    aux = y if c.act == _TANH else z
    return y + x.resid[:c.live].to(dt), aux


def evaluate(c, dt=f64, wrong=None, x=None):
    """The case's outputs over the live rows evaluated in dt from the stored operands, before the final rounding:
    dict C, aux, stats ([live, N / 32, 2]), mean, rstd (those the form has). dt = fp64 is the reference of every form
    but the producer's statistics (those follow the STORED C: producer_stats); fp32 the plain restatement, whose
    producer statistics are those of its own bf16 C."""
    x = x or c.inputs()
    live, K = c.live, c.K
    A, B = x.A[:live], x.B
    if c.form == "producer":
        acc = x.acc[:live] if dt == f64 else A.to(dt) @ B.to(dt).t()
        pre = torch.tensor(c.alpha, dtype=dt) * acc + x.bias.to(dt)
        v = pre + x.resid[:live].to(dt)
        src = {"unrounded": v, "before_resid": pre.to(bf).to(dt)}.get(wrong, v.to(bf).to(dt))
        return {"C": v, "stats": producer_stats(src, dt, wrong)}
    out = {}
    if c.form == "fused":
        mean, M2 = row_stats(A, dt, wrong)
        rstd = rstd_of(M2, K, EPS, wrong)
        a = ((A.to(dt) - mean[:, None]) * rstd[:, None]) * x.gamma.to(dt) + x.beta.to(dt)
        if c.in_dt == bf and wrong != "a_unrounded":
            a = a.to(bf).to(dt)
        z = a @ B.to(dt).t() + x.bias.to(dt)
    else:
        if c.form == "fold":
            mean, M2 = row_stats(A, dt, wrong)
        else:
            mean, M2 = combine((x.stats if dt == f64 else x.stats_given)[:live], dt, wrong)
        rstd = rstd_of(M2, K, EPS, wrong)
        acc = x.acc[:live] if dt == f64 else A.to(dt) @ B.to(dt).t()
        if wrong == "act_first":
            acc = act_ref(c.act, acc)
        m, r, ws, b = mean[:, None], rstd[:, None], x.wsum.to(dt), x.bias.to(dt)
        z = (r * acc - m * ws + b if wrong == "scale_acc_only" else r * (acc - m * ws + b) if wrong == "bias_inside"
             else r * (acc - m * ws) + b)
        if c.rows_out:
            out["mean"], out["rstd"] = mean, rstd
    out["C"], out["aux"] = _tail(c, x, z, dt, wrong)
    return out


def producer_stats(v, dt=f64, wrong=None):
    """(mean, M2) per row and 32-column group of v [rows, N] in dt; wrong: a deliberately wrong producer."""
    rows, N = v.shape
    if wrong == "shift8":
        v = torch.roll(v, -8, dims=1)
    g = v.to(dt).reshape(rows, N // 32, 32)
    n = {"n31": 31.0, "n33": 33.0}.get(wrong, 32.0)
    s = g[..., :24].sum(-1) if wrong == "miss_lane" else g.sum(-1)
    mean = s / n
    return torch.stack([mean, ((g - mean[..., None]) ** 2).sum(-1)], -1)


# ------------------------------------------------------------------------------------------------ bounds

def _drstd_rel(dvar, var):
    return (1 - (dvar / var).clamp(max=0.75)) ** -0.5 - 1 + MARGIN * 4 * U


def producer_stat_bounds(stored):
    """fp64 (ref [rows, G, 2], bound mean_g, bound M2_g) of the statistics of the stored C [rows, N]."""
    rows, N = stored.shape
    g = stored.double().reshape(rows, N // 32, 32)
    ref = group_stats(stored)
    dmean = 10 * U * g.abs().sum(-1) / 32
    dev = (g - ref[..., :1]).abs().sum(-1)
    dm2 = 13 * U * ref[..., 1] + 2 * dev * dmean + 32 * dmean ** 2
    return ref, MARGIN * dmean, MARGIN * dm2


def consumer_stat_bounds(st, K, dmg=None, dm2g=None):
    """fp64 (mean, rstd, dmean, drstd / rstd) per row from the group statistics st [rows, G, 2] (fp32 as given, or the
    exact fp64 ones of a chained case with the producer's bounds dmg / dm2g [rows, G])."""
    mean, M2 = combine(st, f64)
    mg = st[..., 0].double()
    G = mg.shape[1]
    zero = torch.zeros_like(mg)
    dmg, dm2g = (zero if dmg is None else dmg), (zero if dm2g is None else dm2g)
    dmean = MARGIN * (G / 2 + 2) * U * mg.abs().sum(-1) / G + dmg.mean(-1)
    dev = (mg - mean[:, None]).abs()
    e = dmean[:, None] + MARGIN * U * dev + dmg
    dM2 = MARGIN * (G + 8) * U * M2 + 32 * (2 * dev * e + e * e).sum(-1) + dm2g.sum(-1)
    var = M2 / K + EPS
    dvar = dM2 / K + MARGIN * 2 * U * var
    return mean, rstd_of(M2, K, EPS), dmean, _drstd_rel(dvar, var)


def fold_stat_bounds(A, frag):
    """The same four from the stored A rows (fold / fused forms, skinny kernel); frag: the one-pass fragment path."""
    x = A.double()
    K = x.shape[1]
    mean, M2 = row_stats(x, f64)
    var = M2 / K
    if frag:
        n, d = K / 32 + 11, x - x[:, :1]
        dmean = MARGIN * U * (n * d.abs().sum(-1) / K + mean.abs())
        dvar = MARGIN * (n + 3) * U * (var + 2 * (mean - x[:, 0]) ** 2)
    else:
        n = K / 16 + 5
        dmean = MARGIN * n * U * x.abs().sum(-1) / K
        dvar = MARGIN * (n + 2) * U * var + 2 * dmean * (x - mean[:, None]).abs().sum(-1) / K + dmean ** 2
    return mean, rstd_of(M2, K, EPS), dmean, _drstd_rel(dvar + MARGIN * 2 * U * (var + EPS), var + EPS)


def _tail_bounds(c, x, z, dz):
    """(ref C, bound C, ref aux, bound aux) from the fp64 pre-activation and its bound: gemm_epi_refs.bounds's
    forward tail (activation, aux, residual; no beta)."""
    r16 = R16 if c.c_dt == bf else 0.0
    y = act_ref(c.act, z)
    term = 0.0 if c.act in R.EXACT_ACTS else ACT_REL * y.abs() + ACT_ABS * z.abs().clamp(min=1)
    b = R.L_ACT[c.act] * dz + term
    aux = y if c.act == _TANH else z
    aux_b = r16 * aux.abs() + (b if c.act == _TANH else dz)
    r = x.resid[:c.live].double()
    ref = y + r
    return ref, r16 * ref.abs() + b + R.R32 * (y.abs() + r.abs()), aux, aux_b


def boundary_share(c, x=None):
    """Share of the elements of a (fused form, bf16 inputs) whose fp64 value lies within da of a bf16 boundary: (over
    all rows, over the random rows)."""
    return _fused_terms(c, x or c.inputs())[3]


def _fused_terms(c, x):
    live = c.live
    A = x.A[:live].double()
    mean, rstd, dmean, drel = fold_stat_bounds(x.A[:live], c.frag)
    gam, bet = x.gamma.double(), x.beta.double()
    xc = A - mean[:, None]
    a = (xc * rstd[:, None]) * gam + bet
    da = ((rstd[:, None] * gam).abs() * (dmean[:, None] + MARGIN * U * xc.abs()) +
          (xc * rstd[:, None] * gam).abs() * (drel[:, None] + MARGIN * 2 * U) + MARGIN * U * a.abs())
    absB = x.B.double().abs().t()
    if c.in_dt == bf:
        ar = a.to(bf).double()
        flip = torch.maximum(((a + da).to(bf).double() - ar).abs(), ((a - da).to(bf).double() - ar).abs())
        near = (flip > 0).double()
        return ar, flip @ absB + C_ACC[bf] * (ar.abs() @ absB), None, (near.mean().item(), near[NPLANT:].mean().item())
    return a, da @ absB + C_ACC[f32] * (a.abs() @ absB), None, (0.0, 0.0)


def bounds(c, x=None):
    """dict name -> (fp64 reference, bound) of every output of a non-producer case over the live rows."""
    x = x or c.inputs()
    live, K = c.live, c.K
    bias = x.bias.double()
    out = {}
    if c.form == "fused":
        a, dacc, _, _ = _fused_terms(c, x)
        acc = a @ x.B.double().t()
        z = acc + bias
        dz = dacc + MARGIN * U * (acc.abs() + bias.abs())
    else:
        if c.form == "fold":
            mean, rstd, dmean, drel = fold_stat_bounds(x.A[:live], c.frag)
        else:
            mean, rstd, dmean, drel = consumer_stat_bounds(x.stats[:live], K, None if x.dmg is None else x.dmg[:live],
                                                           None if x.dm2g is None else x.dm2g[:live])
            out["mean"], out["rstd"] = (mean, dmean), (rstd, rstd * drel)
        acc, ws = x.acc[:live], x.wsum.double()
        m, r = mean[:, None], rstd[:, None]
        t = r * (acc - m * ws)
        z = t + bias
        dacc = C_ACC[c.in_dt] * x.absacc[:live]
        dz = (r * (dacc + MARGIN * 2 * U * (acc.abs() + (m * ws).abs()) + dmean[:, None] * ws.abs()) +
              t.abs() * (drel[:, None] + MARGIN * U) + MARGIN * U * (t.abs() + bias.abs()))
    ref, b, aux, aux_b = _tail_bounds(c, x, z, dz)
    out["C"], out["aux"] = (ref, b), (aux, aux_b)
    return out


def flips(c, C):
    """Elements of the producer's stored C that are not the bf16 rounding of the fp64 reference (each lies within
    the accumulation error of a rounding boundary, or check() fails): (count on the exact rows 0-23, on the others)."""
    ref = evaluate(c)["C"]
    d = C[:c.live].double() != ref.to(bf).double()
    return int(d[:24].sum()), int(d[24:].sum())


def check(c, got, x=None):
    """Worst ratio of error to bound per output: dict with C and, by form, aux / mean_g / M2_g / mean / rstd. got:
    the launch's outputs (CPU tensors in their stored dtypes; stats [rows, G, 2])."""
    if c.form == "producer":
        ref, b, _, _ = R.bounds(c)
        C = got["C"][:c.live]
        sref, bm, bm2 = producer_stat_bounds(C)
        st = got["stats"][:c.live]
        return {"C": ratio(C, ref, b), "mean_g": ratio(st[..., 0], sref[..., 0], bm), "M2_g": ratio(st[..., 1], sref[..., 1], bm2)}
    return {k: ratio(got[k][:c.live], ref, b) for k, (ref, b) in bounds(c, x).items()}


def stored(c, ev):
    """An evaluation's outputs as a launch would store them (C / aux in the C dtype, statistics and rows in fp32)."""
    return {k: v.to(c.c_dt if k in ("C", "aux") else f32) for k, v in ev.items()}
