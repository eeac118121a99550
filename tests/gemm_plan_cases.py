"""The case list of the GEMM-planner snapshot (tests/golden/gemm_plan_snapshot.json), shared by
tests/test_gemm_plan_cpu.py and tools/gemm_plan_snapshot.py, and the query that plans one case through the public,
host-only entry points (icap_gemm_kernel_name, icap_gemm_plan_info, icap_last_error). The operand pointers are fake:
the planner never dereferences one."""

import ctypes as C

from icap import _lib

STEP_M = (128, 1664, 3200, 3584, 6400, 8320)
STEP_NK = (768, 2304, 3072)
PATHS = (0, 1, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12)
_ACTS = {"gelu_new": _lib.ACT_GELU_NEW, "relu": _lib.ACT_RELU, "quick_gelu": _lib.ACT_QUICK_GELU,
         "tanh": _lib.ACT_TANH, "gelu_erf": _lib.ACT_GELU_ERF}

# the epilogue axes (and K-outer operands, a forced split): name -> the arguments it sets (gemm_args expands flags)
EPILOGUES = [("plain", {})]
EPILOGUES += [(f"act={n}", {"act": v}) for n, v in _ACTS.items()]
EPILOGUES += [(f"dact={n}", {"dact": v}) for n, v in _ACTS.items()]
EPILOGUES += [
    ("act=gelu_new+aux", {"act": _lib.ACT_GELU_NEW, "aux": True}),
    ("ln_stats_out", {"ln": "stats_out"}),
    ("ln_stats_in", {"ln": "stats_in"}),
    ("ln_stats_in+act=gelu_new", {"ln": "stats_in", "act": _lib.ACT_GELU_NEW}),
    ("ln_stats_in+act=quick_gelu", {"ln": "stats_in", "act": _lib.ACT_QUICK_GELU}),
    ("ln_gamma", {"ln": "gamma"}),
    ("ln_wsum", {"ln": "wsum"}),
    ("m_dev", {"m_dev": True}),
    ("m_dev+m_hint=3584", {"m_dev": True, "m_hint": 3584}),
    ("drop=0.1", {"drop_p": 0.1}),
    ("act=relu+drop=0.1", {"act": _lib.ACT_RELU, "drop_p": 0.1}),
    ("c=f32", {"c_dtype": _lib.F32}),
    ("scratch", {"scratch": "ws+tickets"}),
    ("trans_ab", {"trans_ab": 1}),
    ("trans_ab+c=f32+ws", {"trans_ab": 1, "c_dtype": _lib.F32, "scratch": "ws"}),
    ("split_k=3+ws", {"split_k": 3, "scratch": "ws"}),
]


def cases():
    """[(description, M, N, K, arguments)]: every step shape on the automatic path without scratch, with a
    workspace and with workspace + tickets; then one in five of shapes x paths x epilogue axes."""
    out = []
    for M in STEP_M:
        for N in STEP_NK:
            for K in STEP_NK:
                for scratch in (None, "ws", "ws+tickets"):
                    out.append((f"{M}x{N}x{K} p0 scratch={scratch}", M, N, K, {"scratch": scratch}))
    i = 0
    for M in STEP_M:
        for N in STEP_NK:
            for K in STEP_NK:
                for path in PATHS:
                    for e, (name, kw) in enumerate(EPILOGUES):
                        if (i + e) % 5 == 0:
                            out.append((f"{M}x{N}x{K} p{path} {name}", M, N, K, dict(kw, path=path)))
                    i += 1
    return out


def gemm_args(M, N, K, **kw):
    """icap_gemm_args for a bf16 row-major (trans_ab: K-outer) product; flags: aux, m_dev (bool), ln ('stats_out' /
    'stats_in' / 'gamma' / 'wsum'), scratch ('ws' / 'ws+tickets'); every other keyword is a field."""
    kw = dict(kw)
    a = _lib.GemmArgs()
    a.M, a.N, a.K = M, N, K
    a.in_dtype = a.c_dtype = _lib.BF16
    a.A = a.B = a.C = 1 << 20
    trans = kw.get("trans_ab", 0)
    a.lda, a.ldb, a.ldc = (-(-M // 8) * 8, -(-N // 8) * 8, N) if trans else (K, K, N)
    a.alpha = 1.0
    a.ln_eps = 1e-5
    if kw.pop("aux", False):
        a.aux, a.ldaux = 1 << 25, N
    if kw.pop("m_dev", False):
        a.m_dev = 1 << 28
    ln = kw.pop("ln", None)
    if ln == "stats_out":
        a.ln_stats_out = 1 << 26
    if ln == "stats_in":
        a.ln_stats_in = 1 << 26
    if ln in ("stats_in", "wsum"):
        a.ln_wsum = 1 << 27
    if ln == "gamma":
        a.ln_gamma = a.ln_beta = 1 << 27
    scratch = kw.pop("scratch", None)
    if scratch:
        a.workspace, a.workspace_bytes = 1 << 21, 1 << 40
    if scratch == "ws+tickets":
        a.tickets, a.tickets_len = 1 << 22, 1 << 30
    if kw.get("dact", 0):
        a.dact_src, a.ld_dact = 1 << 24, N
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def plan(lib, a):
    """(kernel name, splits, fused) of the plan for `a`, or (error text, None, None) where it is rejected."""
    splits, fused = C.c_int32(-1), C.c_int32(-1)
    rc = lib.icap_gemm_plan_info(C.byref(a), C.byref(splits), C.byref(fused))
    if rc != 0:
        err = lib.icap_last_error().decode()
        assert lib.icap_gemm_kernel_name(C.byref(a)) is None
        return err, None, None
    name = lib.icap_gemm_kernel_name(C.byref(a))
    assert name is not None
    return name.decode(), splits.value, fused.value
