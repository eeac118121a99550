"""The launch trace of the four frozen encoder towers (CLIP vision, ViT, DINOv3, CLIP text), CPU only: every C-ABI
call a `features()` call makes at the real configurations, recorded by tests/dryrun.py and compared call by call
with tests/golden/tower_traces.json (tools/tower_trace.py: scalars and struct fields by value, pointers by first
appearance — leading dimensions and aliasing are part of the trace, addresses are not). The fixture was recorded
from the four per-tower schedules before they were merged into icap/encoder.py, so an equal trace is the proof that
the shared schedule launches exactly what they launched. No tolerance is involved."""

import importlib.util
import json
import os

import pytest

from icap.clip_text import CLIPTextConfig, schedule_gemms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("tower_trace", os.path.join(ROOT, "tools", "tower_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TOOL = _tool()
WANT = json.load(open(TOOL.GOLDEN))


@pytest.fixture(scope="module")
def recorded():
    """{case: (digest, out-of-bounds findings, {(N, K)} of its icap_gemm calls, tower config)}: recorded once."""
    out = {}
    for case, cfg, calls, bad in TOOL.traces():
        nk = {(c[1][0]._obj.N, c[1][0]._obj.K) for c in calls if c[0] == "icap_gemm"}
        out[case] = (TOOL.digest(calls), bad, nk, cfg)
    return out


def test_cases_are_the_committed_ones(recorded):
    assert list(recorded) == list(WANT)
    assert len(WANT) == 22
    # both patch-embedding fronts and both LayerNorm forms of the CLIP tower are in the set
    names = {c: [ln.split()[0] for ln in d["calls"]] for c, d in WANT.items()}
    assert "icap_im2col_patches" in names["clip_b32/bf16_fold"] and "icap_patch_embed" in names["clip_l14/bf16_fold"]
    assert len(names["clip_b32/bf16_fold"]) < len(names["clip_b32/bf16_nofold"]) == len(names["clip_b32/fp32"])
    assert (len(names["clip_b32/fp32"]), len(names["clip_b32/bf16_fold"])) == (91, 69)
    assert (len(names["vit_b16/fp32"]), len(names["vit_b16/bf16"])) == (90, 88)
    assert (len(names["dinov3_l16/fp32"]), len(names["dinov3_l16/bf16"])) == (197, 196)
    # (300, 32) runs as two chunks: twice the launches of a one-chunk call
    assert len(names["clip_text_b32/bf16/B300_L32"]) == 2 * len(names["clip_text_b32/bf16/B6_L77"])


@pytest.mark.parametrize("case", list(WANT))
def test_trace_equals_fixture(recorded, case):
    got, bad, _, _ = recorded[case]
    want = WANT[case]
    assert not bad, bad[:10]  # every extent of every call inside a live allocation
    for i, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert g == w, f"{case}: call {i} is {g}, the fixture has {w}"
    assert len(got["calls"]) == len(want["calls"])
    assert got["hash"] == want["hash"]


@pytest.mark.parametrize("case", [c for c in WANT if c.startswith("clip_text")])
def test_text_tower_gemms_are_the_listed_forms(recorded, case):
    """The (N, K) of the recorded GEMMs are exactly those of schedule_gemms, the list the plan-cover fixture
    (tests/golden/clip_text_plan_cover.json) is built from: that list cannot drift from the schedule."""
    _, _, nk, cfg = recorded[case]
    assert isinstance(cfg, CLIPTextConfig)
    assert nk == {(N, K) for _, N, K, _, _ in schedule_gemms(cfg)}
