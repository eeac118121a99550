"""The GEMM launch planner (csrc/gemm_plan.cpp) pinned without a GPU: the stand-alone checker's hashes over its sweep,
a readable snapshot replayed through the public host-only queries, and the inputs on which the planner once divided
by zero."""

import json
import os
import re
import subprocess

import pytest

import gemm_plan_cases as gpc
from icap import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpt2-image-captioning_amd", "csrc")
SNAPSHOT = os.path.join(ROOT, "tests", "golden", "gemm_plan_snapshot.json")

# `make -C gpt2-image-captioning_amd/csrc plan_check && gpt2-image-captioning_amd/csrc/build/plan_check` prints both.
# PINNED leaves out the inputs on which the rules divided by zero before the planner was split into small rules (M or
# N = 0; K = 0 on path 11, or on paths 8 / 9 / 12 with split_k > 1): it was recorded from those rules, moved verbatim
# into gemm_plan.cpp, and is unchanged since. ALL includes those inputs.
PINNED = ("80daf59005194f16", 25984512)
ALL = ("d5039a960bf6e0a0", 29360640)
# The third sweep (fp32 / MX / K-outer operands with activations, the LayerNorm hand-off, each under the PlanDiag
# overrides of the diagnostic build): recorded on the planner as it was before its epilogue rules and the launchers
# were derived from gemm_plan.h's table of forms, and unchanged by that.
DIAG = ("6d7b54d04d099b7e", 1119744)
# Every form of the table is planned by some case, but the six 8-phase forms with the LayerNorm hand-off and an fp32 C
# (instantiated; gemm_validate takes the hand-off with a bf16 C only).
COVERAGE = "forms 165 planned 159 unplannable 6"
# The forms only a non-default PlanDiag plans (the diagnostic build): variant 5, 128 x 128 tiles at 4 blocks / CU.
_V5 = "icap::gemm_kernel<%s, %s, 1, 4, 2, 2, 4, 4, false, %d>"
DIAG_ONLY = sorted([_V5 % (ti, tc, k) for ti in ("float", "unsigned short") for tc in ("float", "unsigned short") for k in (0, 1)] +
                   [_V5 % ("unsigned short", "unsigned short", k) for k in (17, 33, 256, 512, 529)])


def test_plan_check_hashes(tmp_path):
    """The checker (host compiler, ASan + UBSan, its own main; nothing is loaded into Python) sweeps about 29 M
    argument combinations at 256 compute units, asserts splits >= 1, splits x nk_split covering K, a non-empty grid
    and block, fused only with tickets, and that the table of forms has the instantiation each plan names — and
    prints one hash over every return code, error text and plan of each sweep, then how many of the table's forms
    were planned (it exits non-zero if one that can be was not) and which only under a PlanDiag override."""
    exe = str(tmp_path / "plan_check")
    subprocess.check_call(["make", "-s", "-C", CSRC, "plan_check", f"PLAN_CHECK={exe}"])
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    got = dict((k, (h, int(n))) for k, h, n in re.findall(r"^(pinned|all|diag) ([0-9a-f]{16}) cases (\d+)$", out, re.M))
    assert got == {"pinned": PINNED, "all": ALL, "diag": DIAG}, out
    assert re.findall(r"^forms .*$", out, re.M) == [COVERAGE], out
    assert sorted(re.findall(r"^diag-only (.*)$", out, re.M)) == DIAG_ONLY and len(DIAG_ONLY) == 13, out


def test_snapshot_through_the_public_queries():
    """icap_gemm_kernel_name / icap_gemm_plan_info answer every case of gemm_plan_cases.cases() as recorded in
    tests/golden/gemm_plan_snapshot.json (tools/gemm_plan_snapshot.py regenerates it; recorded from the library before
    the planner was restructured)."""
    lib = _lib.load()
    snap = json.load(open(SNAPSHOT))
    cases = gpc.cases()
    assert len(cases) == len(snap["cases"]) > 3000
    wrong = []
    for (desc, M, N, K, kw), (sdesc, idx, splits, fused) in zip(cases, snap["cases"]):
        assert desc == sdesc
        want = (snap["names"][idx], splits, fused) if idx >= 0 else (snap["errors"][-idx - 1], None, None)
        got = gpc.plan(lib, gpc.gemm_args(M, N, K, **kw))
        if got != want:
            wrong.append((desc, got, want))
    assert not wrong, f"{len(wrong)} of {len(cases)} plans changed, first: {wrong[:3]}"


@pytest.mark.parametrize("kw", [
    dict(path=11, trans_ab=1),                                      # K-outer split-role kernel: nk / splits
    dict(path=11, trans_ab=1, split_k=3, scratch="ws"),
    dict(path=8, split_k=3, scratch="ws"),                          # the forced-split ring paths
    dict(path=9, split_k=3, scratch="ws"),
    dict(path=12, split_k=3, scratch="ws"),
], ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_k_zero_is_an_argument_error(kw):
    lib = _lib.load()
    a = gpc.gemm_args(3584, 768, 0, **kw)
    assert gpc.plan(lib, a) == ("icap_gemm: K must be positive", None, None)


@pytest.mark.parametrize("M,N", [(0, 768), (3584, 0), (0, 0)])
@pytest.mark.parametrize("kw", [
    dict(path=11, trans_ab=1, scratch="ws"),                        # CUs / tiles
    dict(trans_ab=1, scratch="ws"),                                 # 320 blocks / tiles
    dict(scratch="ws+tickets", ln="stats_out"),                     # 2 CUs / tiles (not skinny: the hand-off)
], ids=["path11", "kout", "fusable"])
def test_empty_product_plans_one_split(M, N, kw):
    """M = 0 or N = 0 (icap_gemm returns before planning) through the two query entry points: a plan, splits = 1."""
    lib = _lib.load()
    name, splits, fused = gpc.plan(lib, gpc.gemm_args(M, N, 4096 if "ln" not in kw else 1024, **kw))
    assert name.startswith("icap::gemm_kernel<") and (splits, fused) == (1, 0)
