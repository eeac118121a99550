"""fp64 references (CPU tensors), inputs, per-element bounds and the case list of the GEMM epilogue (icap_gemm:
bias, activation / aux, residual, beta, and the backward dact form) on every kernel family. test_gemm_epi_refs_cpu.py
checks the references, the bounds and the planned kernels without a GPU (a plain fp32 evaluation of every case must
stay inside its bound; a deliberately wrong epilogue must not); test_gemm_epilogue_gpu.py checks the kernels.

Reference (include/icap.h "Epilogue order", fp64; dropout stays at p = 0, its sites are dropout_refs.py's):

    forward   z = alpha * acc + bias;  aux = (act == tanh ? act(z) : z);  v = act(z) + resid;  C = beta * C0 + v
    backward  v = alpha * acc * act'(dact_src);                                              C = beta * C0 + v

gelu_new is 0.5 z (1 + tanh(sqrt(2 / pi) (z + 0.044715 z^3))), quick_gelu z sigmoid(1.702 z), gelu_erf z Phi(z)
computed as 0.5 z erfc(-z / sqrt 2) (the reference keeps its tail), relu and tanh themselves; the derivatives come
from autograd in fp64, except relu' (z > 0) and tanh', which the library takes from the STORED tanh output a (the aux
of a tanh forward) as 1 - a^2.

Inputs (one generator per (in dtype, C dtype), the same for every kernel family; cached per shape with their fp64
products). The first P = 16 rows are planted: row m of A is the unit vector e_m, so acc[m, n] = B[n, m] exactly, and
B[n, k < P] = 2 * GRID[(n + k) % len(GRID)] with alpha = 0.5 (a power of two), so alpha * acc is a GRID value with no
rounding at all. GRID is bf16-exact and spans [-12, 12]: +-0, +-2^-20, five bf16 neighbours of -0.75 (the minimum of
the GELUs, the sign change of quick_gelu'), +-1, the erf tail -3.5 ... -6.5 where 1 + erff cancels, -7.1875, the
points 4.25 / 9.75 / 10 past which 1 + exp(-t) is 1 in fp32 for gelu_new / quick_gelu, and -10.25 where gelu_new's
exponential overflows fp32. bias is 0 on the columns with (n / 8) even, so there z is the GRID value exactly and the
activation is probed through the real kernel with no accumulation error; on the other columns z carries the one
rounding of the fma. dact_src carries GRID on the planted rows too (shifted, so every pairing with acc occurs), and
with an fp32 C values of GRID * (1 + 2^-12), exact in fp32 only. The remaining rows are random: A ~ N(0, 1) with
zeros under the planted columns, B ~ N(0, 2.4^2 / K), bias ~ N(0, 0.9^2): z ~ N(0, 1.5^2).

Bounds, per element; every check returns the worst ratio of error to bound (<= 1 passes), never a max-norm:

    C forward   |d| <= r16 |ref| + L_act dz + act_term(z) + 2^-23 (|act(z)| + |resid|) [resid]
                                 + 2^-23 (|beta C0| + |v|) [beta]
    aux         |d| <= r16 |ref| + dz                        (tanh: + dz replaced by L dz + act_term)
    C backward  |d| <= r16 |ref| + |alpha| dacc |act'| + |alpha acc| (ACT_REL |act'| + ACT_ABS max(1, |src|))
                                 + 2^-23 |v| + 2^-23 (|beta C0| + |v|) [beta]
    act_term(z) = ACT_REL |act(z)| + ACT_ABS max(1, |z|)     (0 for relu and for no activation: both are exact)

  r16 = 2^-8 for a bf16 output (the one rounding), 0 for fp32. dacc = C_ACC |A| . |B|^T and dz = |alpha| dacc +
  C_ACC |bias| with C_ACC = 2e-6 for fp32 inputs, 1e-5 for bf16 inputs (test_kernels_gpu.test_gemm_plain's); on the
  planted rows dacc = 0 and dz = 2^-24 (|alpha acc| + |bias|), the fma's rounding, 0 where bias is 0. L_act = sup
  |act'|: 1 for relu / tanh, 1.13 for the three GELUs (gelu_new 1.1290, gelu_erf 1.1289, quick_gelu 1.0998; the CPU test
  re-measures the suprema on a grid).

Constants, derived for the device's evaluation (csrc/common.h act_fwd / act_bwd read for WHICH intrinsics run, not
for their formulae): the sigmoid forms are z * rcp(1 + __expf(-t)). __expf(x) is v_exp_f32 (1 ulp = 2^-23) of
x * log2(e), whose rounding adds |x| 2^-23 relative; the argument t (a cubic for gelu_new) adds about 3 roundings,
another |t| 1.5 2^-23; 1 + e rounds (2^-24), v_rcp_f32 is 1 ulp, the product with z rounds (2^-24). With s =
1 / (1 + e): d s / s = 2^-23 (2 + (1 - s) (1 + 2.5 |t|)). The parts without |t| are relative: at most 4 * 2^-23. The
|t| part is |z| s (1 - s) |t| 2.5 2^-23 <= 0.224 * 2.5 * 2^-23 |z| = 0.56 * 2^-23 |z| (s (1 - s) |t| peaks at 0.224,
|t| = 1.54): absolute, and no relative bound can hold it in the negative tail, where s ~ e^-|t|. The erf GELU is
0.5 z (1 + erff(z / sqrt 2)): HIP documents erff to 4 ulp, so 1 + erff is off by up to (4 + 1) 2^-24 ABSOLUTE and
the result by 1.25 * 2^-23 |z|, whatever Phi(z) is; tanhf is documented to 2 ulp. The derivatives are sums of such
terms of size <= 1 each (s + 2 a s (1 - s) u'(a), Phi + a phi): the same relative parts, the |t|-scaled part 2 |a| u'
s (1 - s) |t| 2^-22 <= 0.52 * 2^-22 (measured on a grid of a), the erf form 2.5 * 2^-24 + 0.23 * 2^-23; they cancel at
the derivative's zero (a ~ -0.75), which the absolute part also covers. So: relative 4 * 2^-23, absolute 1.25 * 2^-23
per max(1, |z|). With the 4 x margin loss_refs.py takes over its derivation:

    ACT_REL = 2^-19 (1.9e-6)        ACT_ABS = 5 * 2^-23 (6.0e-7)

  Nothing is tuned to a kernel's output. Two of the bound's terms are reached by a correct evaluation by construction:
  the rounding of a bf16 store (r16) and, on the planted rows, the fma's half ulp in aux; the ratios of those elements
  sit just under 1 whatever the arithmetic did. The arithmetic's own figure is the ratio of C with an fp32 C
  (check(parts=True)). Worst ratios of a plain fp32 torch evaluation on the CPU (test_plain_fp32_inside_bounds, all
  148 cases): 1.000 over everything (a bf16 store's rounding) and over aux; C with an fp32 C: relu + resid 0.604,
  gelu_new 0.128, quick_gelu 0.151, gelu_erf 0.128, tanh 0.122 (the forwards carry a residual, whose add's half ulp
  against 2^-23 is most of these), gelu_new' 0.410 (with beta; 0.16 without), quick_gelu' 0.123, relu' 0.123,
  tanh' 0.100, gelu_erf' 0.087; the residual-free fp32 forwards (the activation alone): gelu_new 0.082, quick_gelu
  0.083, gelu_erf 0.086, tanh 0.075 (relu: the fma's half ulp, 0.995).

Case list: CASES, one entry per (kernel family, epilogue kind, in dtype, C dtype [, layout]); each names the kernel
instantiation it must plan to and launch (variant template integers + the ACT integer, as test_gemm_roles_gpu._name).
Shapes are the smallest at which each family is eligible (csrc/gemm_plan.cpp) with a partial row tile, a partial
column tile and a K tail: 300 x 264 x 200 for the ring families and the 8-phase kernels (M >= 256), 100 x 130 x 200
for variant 4 and the skinny kernel (M <= 128), 130 x 8136 x 64 for variant 13 (256 tiles of 128 x 64), 200 x 132 x
1544 for variant 0's in-launch split with tickets (>= 24 K stages, N % 4 == 0), K = 1096 for the long-K rings.

Coverage. The 23 specialised non-LayerNorm kinds of the table (gemm_plan.h TILE_VARIANTS, G8P_EPI) for bf16 row-major
operands with a bf16 C are all planned and launched. With an fp32 C the table instantiates a specialised kind for the
8-phase kernel only (G8P_EPI has f32_c_plain = false; every TILE_VARIANTS row keeps the default f32_c_plain = true, "an
fp32 C has ACT_OFF / ACT_ANY only", and gemm_plan.cpp epilogue_kind returns the dispatching kind for wide_c): the 4
8-phase pairs are covered as specialised kinds; the other 19 (kind, fp32 C) pairs -- variants 0, 4, 13, 22, 26, 28 --
do not exist as kernels, so the list runs the same arguments with an fp32 C and pins them to the dispatching
instantiation they plan to (kind "any"; test_gemm_epi_refs_cpu.test_coverage counts 27 + 19). Variant 5 is planned
only by the diagnostic build (test_gemm_plan_cpu.DIAG_ONLY) and is left out. The LayerNorm hand-off kinds (and the
skinny kernel's fold and fused LayerNorm) are gemm_ln_refs.py's.

MEASURED on an MI355X (test_gemm_epilogue_gpu.py, every element of every case; "all" = C and aux of every launch of
the family, "C f32" = C of its fp32-C launches, the arithmetic's own figure):
    family   all    C f32 | family   all    C f32 | family    all    C f32 | family    all    C f32
    v4       0.995  0.410 | v22      0.995  0.324 | g8p128    0.995  0.324 | v0_f32in  0.995  -
    v4_f32in 0.990  0.990 | v24      0.995  -     | g8p256    0.995  0.324 | v14       0.995  -
    v0       0.987  0.324 | v25      0.995  -     | g256      0.995  -     | v15       0.995  -
    v12      0.995  -     | v26      0.995  0.324 | skinny    0.995  0.995 | v31       0.995  -
    v13      1.000  0.604 | v27      0.995  -     | reduce    0.996  0.077 | v26_n130  0.996  0.368
    v16      0.995  -     | v28      0.995  0.497 | v32       0.995  -     |
  By epilogue with an fp32 C: gelu_new 0.128, quick_gelu 0.151, gelu_erf 0.128, tanh 0.122 (aux 0.050), relu + resid
  0.604; gelu_new' 0.324 without beta (the same planted element on every family) and up to 0.410 with beta,
  quick_gelu' 0.123, gelu_erf' 0.073, tanh' 0.071, relu' 0.084. The residual-free fp32 forwards of v4_f32in /
  skinny (the activation alone, no rounding after it): gelu_new 0.071, quick_gelu 0.067, gelu_erf 0.070, tanh 0.050;
  relu 0.995, which is the fma's half ulp on the planted rows and the "C f32" figure of those two families.
  Sentinels intact and the named kernel launched in all 148 cases.
"""

import functools
import math

import torch

from icap import _lib as L

bf, f32, f64 = torch.bfloat16, torch.float32, torch.float64
SENTINEL = -96.0  # exact in bf16: every element a launch must not touch
ALPHA = 0.5
P = 16            # planted rows
ACT_REL = 2.0 ** -19
ACT_ABS = 5 * 2.0 ** -23
R16 = 2.0 ** -8
R32 = 2.0 ** -23
C_ACC = {f32: 2e-6, bf: 1e-5}
ACTS = {"gelu_new": L.ACT_GELU_NEW, "relu": L.ACT_RELU, "quick_gelu": L.ACT_QUICK_GELU, "tanh": L.ACT_TANH,
        "gelu_erf": L.ACT_GELU_ERF}
ACT_NAME = {v: k for k, v in ACTS.items()}
L_ACT = {L.ACT_NONE: 1.0, L.ACT_RELU: 1.0, L.ACT_TANH: 1.0, L.ACT_GELU_NEW: 1.13, L.ACT_QUICK_GELU: 1.13,
         L.ACT_GELU_ERF: 1.13}
EXACT_ACTS = (L.ACT_NONE, L.ACT_RELU)

_NB = [-0.75 + i * 2.0 ** -8 for i in (-2, -1, 0, 1, 2)]
GRID = [0.0, -0.0, 2.0 ** -20, -2.0 ** -20, 1.0, -1.0, 0.5, -0.5, 0.25, -0.25, 0.125, -0.125, 1.5, -1.5, 2.0, -2.0,
        3.0, -3.0, -3.5, -4.0, -4.5, -5.0, -5.5, -6.0, -6.5, 3.5, 4.25, 4.5, -4.25, 6.0, -7.1875, 7.1875, 8.0, -8.0,
        9.75, -9.75, 10.0, -10.0, 10.25, -10.25, 12.0, -12.0, 0.75, 0.0625, -0.0625] + _NB   # 50 values


def dt_name(dt):
    return "bf16" if dt == bf else "f32"


# ------------------------------------------------------------------------------------------------ activations

def act_ref(a, z, wrong=None):
    """act(z) in z's dtype (fp64: the reference; fp32: the plain evaluation). wrong: a deliberately wrong formula."""
    if a == L.ACT_NONE:
        return z
    if wrong == "swap_gelus":
        a = {L.ACT_GELU_NEW: L.ACT_GELU_ERF, L.ACT_GELU_ERF: L.ACT_GELU_NEW}.get(a, a)
    if a == L.ACT_GELU_NEW:
        c3 = 0.044715 if wrong != "gelu_new_cubic" else 0.044715 / 3  # (only meaningful through the derivative)
        return 0.5 * z * (1 + torch.tanh(math.sqrt(2 / math.pi) * (z + c3 * z ** 3)))
    if a == L.ACT_RELU:
        return torch.relu(z)
    if a == L.ACT_QUICK_GELU:
        return z * torch.sigmoid((1.7 if wrong == "quick_1.7" else 1.702) * z)
    if a == L.ACT_TANH:
        return torch.tanh(z)
    if a == L.ACT_GELU_ERF:
        return 0.5 * z * torch.special.erfc(-z / math.sqrt(2))
    raise ValueError(a)


def dact_ref(a, s, wrong=None):
    """act'(.) as the backward epilogue takes it from the stored operand s (relu: z or relu(z); tanh: the tanh
    output; the GELUs: the pre-activation), in s's dtype."""
    if a == L.ACT_NONE:
        return torch.ones_like(s)
    if a == L.ACT_RELU:
        return (s >= 0 if wrong == "relu_at_0" else s > 0).to(s.dtype)
    if a == L.ACT_TANH:
        return 1 - s * s
    if wrong == "gelu_new_cubic" and a == L.ACT_GELU_NEW:  # du/dz with 0.044715 in place of 3 * 0.044715
        c = math.sqrt(2 / math.pi)
        t = torch.tanh(c * (s + 0.044715 * s ** 3))
        return 0.5 * (1 + t) + 0.5 * s * (1 - t * t) * c * (1 + 0.044715 * s * s)
    x = s.clone().requires_grad_(True)
    return torch.autograd.grad(act_ref(a, x, wrong).sum(), x)[0]


# ------------------------------------------------------------------------------------------------ inputs

class Inputs:
    pass


@functools.lru_cache(maxsize=None)
def inputs(in_dt, c_dt, M, N, K):
    """The operands of one shape (CPU tensors in their storage dtypes) and their fp64 products, never modified."""
    assert M > P and K >= P
    g = torch.Generator().manual_seed(1000 * M + 10 * N + K + (3 if in_dt == bf else 0) + (5 if c_dt == bf else 0))
    grid = torch.tensor(GRID, dtype=f64)
    G = len(GRID)
    n = torch.arange(N)
    A = torch.randn((M, K), generator=g, dtype=f64)
    A[:, :P] = 0
    A[:P] = 0
    A[torch.arange(P), torch.arange(P)] = 1
    B = torch.randn((N, K), generator=g, dtype=f64) * (2.4 / math.sqrt(K))
    B[:, :P] = grid[(n[:, None] + torch.arange(P)[None, :]) % G] / ALPHA
    bias = torch.randn(N, generator=g, dtype=f64) * 0.9
    bias[(n // 8) % 2 == 0] = 0
    resid = torch.randn((M, N), generator=g, dtype=f64)
    dsrc = torch.randn((M, N), generator=g, dtype=f64) * 1.5
    dsrc[:P] = grid[(n[None, :] + 3 * torch.arange(P)[:, None] + 7) % G]
    if c_dt == f32:
        dsrc[P // 2:P] *= 1 + 2.0 ** -12
    C0 = torch.randn((M, N), generator=g, dtype=f64)
    x = Inputs()
    x.in_dt, x.c_dt, x.M, x.N, x.K = in_dt, c_dt, M, N, K
    x.A, x.B = A.to(in_dt), B.to(in_dt)
    x.bias = bias.to(f32)
    x.resid, x.dsrc, x.C0 = resid.to(c_dt), dsrc.to(c_dt), C0.to(c_dt)
    assert torch.equal(x.B[:, :P].double(), B[:, :P]) and (c_dt == f32 or torch.equal(x.dsrc[:P].double(), dsrc[:P]))
    x.acc = x.A.double() @ x.B.double().t()
    x.absacc = x.A.double().abs() @ x.B.double().abs().t()
    x.absacc[:P] = 0  # planted rows: one exact product
    x.planted = torch.zeros((M, 1), dtype=torch.bool)
    x.planted[:P] = True
    assert torch.equal(x.acc[:P], x.B[:, :P].double().t())
    return x


# ------------------------------------------------------------------------------------------------ cases

# variant id -> the template integers NST, MINB, WM, WN, TM, TN of its kernel name (restated, not read from the table)
FORMS = {0: "2, 2, 2, 2, 4, 4", 4: "1, 3, 2, 2, 4, 4", 12: "2, 3, 2, 2, 4, 2", 13: "1, 4, 2, 2, 4, 2",
         14: "2, 2, 2, 2, 4, 4", 15: "1, 3, 2, 2, 4, 4", 16: "4, 1, 2, 2, 4, 4", 22: "3, 1, 4, 2, 4, 4",
         24: "2, 2, 4, 1, 3, 4", 25: "4, 1, 4, 1, 3, 4", 26: "3, 1, 2, 2, 4, 8", 27: "5, 1, 2, 2, 3, 4",
         28: "2, 1, 2, 4, 6, 4", 31: "4, 1, 2, 2, 4, 4", 32: "4, 1, 2, 2, 5, 4"}
KOUT = (14, 15, 31)
ROLES = (26, 27, 28, 31, 32)
ACT_OFF, ACT_ANY, ACT_FWD, ACT_BWD = 0, 1, 16, 32


def _ctype(dt):
    return "unsigned short" if dt == bf else "float"


def tile_name(v, in_dt, c_dt, actk):
    return (f"icap::gemm_kernel<{_ctype(in_dt)}, {_ctype(c_dt)}, {FORMS[v]}, {'true' if v in KOUT else 'false'}, "
            f"{actk}{', true' if v in ROLES else ''}>")


# family -> (ops.gemm keywords, shape (M, N, K), how its kernel is named)
S_RING, S_LONG, S_SMALL, S_N13, S_FUSED = (300, 264, 200), (300, 264, 1096), (100, 130, 200), (130, 8136, 64), \
    (200, 132, 1544)
FAMILIES = {
    "v4": (dict(tile_only=True, split_k=1), S_SMALL, 4),
    "v12": (dict(tile_only=True, split_k=1), S_RING, 12),
    "v13": (dict(tile_only=True, split_k=1), S_N13, 13),
    "v16": (dict(tile_only=True, split_k=1), S_LONG, 16),
    "v0": (dict(), S_FUSED, 0),                               # automatic: the in-launch split with tickets
    "v0_f32in": (dict(tile_only=True, split_k=1), (200, 130, 520), 0),
    "v4_f32in": (dict(tile_only=True, split_k=1), (200, 130, 200), 4),
    "v22": (dict(r256=True, split_k=1), S_RING, 22),
    "v24": (dict(w192=True, split_k=1), S_RING, 24),
    "v25": (dict(w192=True, split_k=1), S_LONG, 25),
    "v26": (dict(roles=256, split_k=1), S_RING, 26),
    "v27": (dict(roles=96, split_k=1), S_RING, 27),
    "v28": (dict(roles=192, split_k=1), S_RING, 28),
    "v32": (dict(roles=160, split_k=1), S_RING, 32),
    "g8p128": (dict(g8p=128, split_k=1), S_RING, "g8p"),
    "g8p256": (dict(g8p=256, split_k=1), S_RING, "g8p"),
    "g256": (dict(g256=True), S_RING, "g256"),
    "skinny": (dict(), S_SMALL, "skinny"),
    "reduce": (dict(tile_only=True, split_k=3), (200, 132, 200), "reduce"),
    "v15": (dict(trans_ab=True, tile_only=True, split_k=1), S_RING, 15),
    "v14": (dict(trans_ab=True, tile_only=True, split_k=1), S_LONG, 14),
    "v31": (dict(trans_ab=True, roles=1, split_k=1), S_RING, 31),
    "v26_n130": (dict(roles=256, split_k=1), (300, 130, 200), 26),
}


def path_of(kw):
    """ops.gemm's keyword -> icap_gemm_args.path (include/icap.h)."""
    roles = kw.get("roles", 0)
    return (1 if kw.get("tile_only") else 3 if kw.get("g256") else 4 if kw.get("g8p") == 128 else
            5 if kw.get("g8p") == 256 else 6 if kw.get("r256") else 7 if kw.get("w192") else
            {0: 0, 256: 8, 96: 9, 192: 10, 1: 11, 160: 12}[roles])


class Layout:
    """Leading dimensions of C / aux / resid / dact_src (None: contiguous, N) and the element offset of every base
    pointer inside its padded buffer."""

    def __init__(self, name, ldc=None, ldaux=None, ldr=None, ldd=None, off=0):
        self.name, self.ldc, self.ldaux, self.ldr, self.ldd, self.off = name, ldc, ldaux, ldr, ldd, off


PLAIN = Layout("contig")


def layouts(N):
    return [Layout("ld%8", N + 6 + (-(N + 6)) % 8, N + 14 + (-(N + 14)) % 8, N + 22 + (-(N + 22)) % 8,
                   N + 30 + (-(N + 30)) % 8),
            Layout("ld=N+1", N + 1, N + 1, N + 1, N + 1),
            Layout("off1", N + 6 + (-(N + 6)) % 8, N + 14 + (-(N + 14)) % 8, N + 6 + (-(N + 6)) % 8,
                   N + 14 + (-(N + 14)) % 8, off=1)]


class Case:
    def __init__(self, family, in_dt, c_dt, act=0, dact=0, kind="any", beta=0.0, m_dev=False, layout=PLAIN, resid=True):
        self.family, self.in_dt, self.c_dt, self.act, self.dact, self.kind = family, in_dt, c_dt, act, dact, kind
        self.beta, self.layout = beta, layout
        self.kw, (self.M, self.N, self.K), self.named = FAMILIES[family]
        self.trans = bool(self.kw.get("trans_ab"))
        self.live = self.M - 3 if m_dev else self.M
        self.m_dev = m_dev
        self.alpha = ALPHA
        # the forward form carries everything it can: bias, aux, resid; the backward its dact_src
        self.bias = self.aux = not dact
        self.resid = resid and not dact
        d = f"F-{ACT_NAME[act]}" if act else f"B-{ACT_NAME[dact]}"
        self.name = (f"{family}-{d}-{kind}-{dt_name(in_dt)}-{dt_name(c_dt)}" + (f"-beta{beta:g}" if beta else "") +
                     ("" if resid else "-nores") + ("-mdev" if m_dev else "") +
                     (f"-{layout.name}" if layout is not PLAIN else ""))

    def __repr__(self):
        return self.name

    def actk(self):
        if self.named == "reduce":
            return ACT_OFF  # the epilogue runs in the reduce pass
        if self.kind == "any":
            return ACT_ANY
        return ACT_FWD + self.act if self.act else ACT_BWD + self.dact

    def kernel(self):
        """The instantiation the launch must plan to (and, on the GPU, record)."""
        if self.named == "g256":
            return f"icap::gemm256_kernel<{_ctype(self.c_dt)}>"
        if self.named == "g8p":
            return f"icap::gemm8p_kernel<{_ctype(self.c_dt)}, {self.kw['g8p']}, {self.actk()}>"
        if self.named == "skinny":  # one 16-column slab per block; 6 k-steps in flight (fp32) / 3 (bf16, K = 200)
            return (f"icap::gemm_skinny_kernel<{_ctype(self.in_dt)}, {_ctype(self.c_dt)}, 1, 2, "
                    f"{6 if self.in_dt == f32 else 3}>")
        v = 4 if self.named == "reduce" else self.named
        return tile_name(v, self.in_dt, self.c_dt, self.actk())

    def inputs(self):
        return inputs(self.in_dt, self.c_dt, self.M, self.N, self.K)

    def lds(self):
        lay, N = self.layout, self.N
        return lay.ldc or N, lay.ldaux or N, lay.ldr or N, lay.ldd or N


# the 23 specialised non-LayerNorm kinds of the table: family -> [(forward act, backward act)]
_GN, _QG, _RELU, _ERF, _TANH = (ACTS[k] for k in ("gelu_new", "quick_gelu", "relu", "gelu_erf", "tanh"))
SPECIALISED = {
    "v0": [(_GN, 0), (0, _GN)],
    "v4": [(_GN, 0), (_QG, 0), (_ERF, 0), (0, _GN)],
    "v13": [(_RELU, 0), (0, _RELU)],
    "v22": [(_GN, 0), (_QG, 0), (0, _GN)],
    "v26": [(_GN, 0), (_QG, 0), (0, _GN)],
    "v28": [(_GN, 0), (_QG, 0), (_RELU, 0), (0, _GN), (0, _RELU)],
    "g8p128": [(_GN, 0), (0, _GN)],
    "g8p256": [(_GN, 0), (0, _GN)],
}
F32_C_SPECIALISED = ("g8p128", "g8p256")  # the only rows of the table with f32_c_plain = false
DISPATCH_FAMILIES = ["v4", "v12", "v13", "v16", "v0", "v0_f32in", "v22", "v24", "v25", "v26", "v27", "v28", "v32",
                     "g8p128", "g8p256", "g256", "skinny", "reduce", "v15", "v14", "v31"]


def _cases():
    out = []
    # every specialised kind, bf16 operands, a bf16 C and an fp32 C (tile variants: the dispatching kind, see above)
    for fam, kinds in SPECIALISED.items():
        for a, d in kinds:
            for c_dt in (bf, f32):
                spec = c_dt == bf or fam in F32_C_SPECIALISED
                out.append(Case(fam, bf, c_dt, act=a, dact=d, kind="spec" if spec else "any"))
    # base tile path and skinny kernel: all five activations, forward and backward, fp32 in / fp32 C; the forwards
    # also without a residual (no rounding after the activation: the sharpest probe of it)
    for fam in ("v4_f32in", "skinny"):
        for a in ACTS.values():
            out.append(Case(fam, f32, f32, act=a))
            out.append(Case(fam, f32, f32, act=a, resid=False))
            out.append(Case(fam, f32, f32, dact=a))
    # the dispatching kind on every family: tanh forward and a derivative no family specialises (bf16 C)
    for fam in DISPATCH_FAMILIES:
        in_dt = f32 if fam.endswith("f32in") else bf
        out.append(Case(fam, in_dt, bf, act=_TANH))
        out.append(Case(fam, in_dt, bf, dact=_QG))
    out.append(Case("reduce", bf, f32, act=_ERF))
    out.append(Case("reduce", bf, f32, dact=_ERF))
    # layout axes on the base tile path and one ring family: N = 130, m_dev = M - 3, padded views
    for fam in ("v4", "v26_n130"):
        for lay in layouts(FAMILIES[fam][1][1]):
            out.append(Case(fam, bf, bf, act=_GN, kind="spec", m_dev=True, layout=lay))
            out.append(Case(fam, bf, bf, dact=_QG, m_dev=True, layout=lay))
            out.append(Case(fam, bf, f32, act=_QG, beta=0.5, m_dev=True, layout=lay))
            out.append(Case(fam, bf, f32, dact=_GN, beta=1.0, m_dev=True, layout=lay))
            if lay.name == "ld%8":  # (the other beta of each form, once)
                out.append(Case(fam, bf, f32, act=_QG, beta=1.0, m_dev=True, layout=lay))
                out.append(Case(fam, bf, f32, dact=_GN, beta=0.5, m_dev=True, layout=lay))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


CASES = _cases()


def plan_args(c):
    """The icap_gemm_args ops.gemm builds for the case, with fake pointers (gemm_plan_cases.gemm_args): the planner
    reads sizes, leading dimensions and pointer alignment only."""
    from gemm_plan_cases import gemm_args

    ldc, ldaux, ldr, ldd = c.lds()
    es = 2 if c.c_dt == bf else 4
    off = c.layout.off * es
    kw = dict(in_dtype=L.BF16 if c.in_dt == bf else L.F32, c_dtype=L.BF16 if c.c_dt == bf else L.F32, act=c.act,
              dact=c.dact, alpha=c.alpha, beta=c.beta, path=path_of(c.kw), split_k=c.kw.get("split_k", 0),
              scratch="ws+tickets", trans_ab=1 if c.trans else 0, m_dev=c.m_dev)
    a = gemm_args(c.M, c.N, c.K, **kw)
    a.C, a.ldc = (1 << 20) + off, ldc
    if c.bias:
        a.bias = 1 << 23
    if c.aux:
        a.aux, a.ldaux = (1 << 25) + off, ldaux
    if c.resid:
        a.resid, a.ldr = (1 << 29) + off, ldr
    if c.dact:
        a.dact_src, a.ld_dact = (1 << 24) + off, ldd
    return a


# ------------------------------------------------------------------------------------------------ reference + bounds

def evaluate(c, dt=f64, wrong=None):
    """(C, aux) of the case's live rows evaluated in dtype dt from the stored operands, before the final rounding to
    the C dtype. dt = fp64 is the reference, fp32 the plain evaluation; wrong names a deliberately wrong epilogue."""
    x = c.inputs()
    live = c.live
    acc = x.acc[:live] if dt == f64 else (x.A[:live].to(dt) @ x.B.to(dt).t())
    alpha = torch.tensor(c.alpha, dtype=dt)
    aux = None
    if c.dact:
        s = x.dsrc[:live].to(dt)
        v = (acc if wrong == "bwd_no_alpha" else alpha * acc) * dact_ref(c.dact, s, wrong)
    else:
        bias = x.bias.to(dt) if c.bias else torch.zeros(c.N, dtype=dt)
        z = alpha * (acc + bias) if wrong == "alpha_times_sum" else alpha * acc + bias
        r = x.resid[:live].to(dt) if c.resid else None
        if wrong == "resid_first" and r is not None:
            z = z + r
        y = act_ref(c.act, z, wrong)
        aux = y if c.act == _TANH else z
        if wrong == "aux_is_act" and c.act not in (0, _TANH):
            aux = y
        if wrong == "aux_is_pre" and c.act == _TANH:
            aux = z
        v = y if r is None or wrong == "resid_first" else y + r
    if c.beta:
        c0 = x.C0[:live].to(dt)
        v = c0 + c.beta * v if wrong == "beta_on_v" else c.beta * c0 + v
    return v, (aux if c.aux else None)


def bounds(c):
    """fp64 (ref C, bound C, ref aux, bound aux) over the live rows (aux: None where the case has none)."""
    x = c.inputs()
    live = c.live
    r16 = R16 if c.c_dt == bf else 0.0
    acc, absacc, planted = x.acc[:live], x.absacc[:live], x.planted[:live]
    a = abs(c.alpha)
    dacc = C_ACC[c.in_dt] * absacc  # (0 on the planted rows)
    ref, aux = evaluate(c)
    if c.dact:
        s = x.dsrc[:live].double()
        d = dact_ref(c.dact, s)
        v = c.alpha * acc * d
        b = a * dacc * d.abs() + R32 * v.abs()
        if c.dact not in EXACT_ACTS:
            b = b + (a * acc).abs() * (ACT_REL * d.abs() + ACT_ABS * s.abs().clamp(min=1))
        aux_b = None
    else:
        bias = x.bias.double() if c.bias else torch.zeros(c.N, dtype=f64)
        z = c.alpha * acc + bias
        dz = torch.where(planted, torch.where(bias == 0, 0.0, 2.0 ** -24 * ((c.alpha * acc).abs() + bias.abs())),
                         a * dacc + C_ACC[c.in_dt] * bias.abs())
        y = act_ref(c.act, z)
        term = 0.0 if c.act in EXACT_ACTS else ACT_REL * y.abs() + ACT_ABS * z.abs().clamp(min=1)
        b = L_ACT[c.act] * dz + term
        aux_b = None
        if c.aux:
            aux_b = r16 * aux.abs() + (b if c.act == _TANH else dz)
        v = y
        if c.resid:
            r = x.resid[:live].double()
            b = b + R32 * (y.abs() + r.abs())
            v = y + r
    if c.beta:
        b = b + R32 * ((c.beta * x.C0[:live].double()).abs() + v.abs())
    return ref, r16 * ref.abs() + b, aux, aux_b


def ratio(got, ref, bound):
    """Worst |got - ref| / bound over every element (inf where an element is not finite or misses a zero bound)."""
    err = (got.double() - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, math.inf, 0.0))
    r = torch.where(torch.isfinite(got.double()), r, math.inf)
    return r.max().item()


def check(c, C, aux=None, parts=False):
    """Worst ratio of the live rows of C (and aux) against the case's bounds; parts: (of C, of aux) apart (aux 0
    where the case has none). With an fp32 C the figure of C is the arithmetic's own: the bound of a bf16 store is
    reached by its rounding alone (ratios near 1 whatever the arithmetic did), and so is the planted rows' aux bound,
    which is the fma's half ulp."""
    ref, b, aref, ab = bounds(c)
    w = ratio(C[:c.live], ref, b)
    wa = ratio(aux[:c.live], aref, ab) if c.aux else 0.0
    return (w, wa) if parts else max(w, wa)
