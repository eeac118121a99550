"""The host-side tile choice of icap_gemm_group (csrc/gemm_plan.cpp gemm_group_plan): 128 x 256 tiles when the group then
fits one round of one block per compute unit, the 128 x 128 body otherwise or under the override; products of at most
4 output columns run exchanged on the big tiles. Checked through the stand-alone group_check program (host compiler,
ASan + UBSan, like plan_check) over a table of shapes."""

import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpt2-image-captioning_amd", "csrc")

LAYER = [(3072, 768), (768, 3072), (2304, 768), (768, 768)]
BIAS = [(3072, 1), (768, 1), (2304, 1), (768, 1)]

# (cus, force128, [(M, N), ...]) -> (big, total, swap mask, ["tiles_m x tiles_n", ...])
TABLE = [
    # a mapper layer: 72 + 72 + 54 + 18 = 216 weight-gradient tiles, + 12 + 3 + 9 + 3 = 27 exchanged bias tiles
    ((256, 0, LAYER), (True, 216, 0, ["24x3", "6x12", "18x3", "6x3"])),
    ((256, 0, LAYER + BIAS), (True, 243, 0xF0, ["24x3", "6x12", "18x3", "6x3", "1x12", "1x3", "1x9", "1x3"])),
    # the override keeps the 128 x 128 body: 432 + 54 tiles
    ((256, 1, LAYER + BIAS), (False, 486, 0, ["24x6", "6x24", "18x6", "6x6", "24x1", "6x1", "18x1", "6x1"])),
    # a device too small for one round of the layer
    ((240, 0, LAYER + BIAS), (False, 486, 0, ["24x6", "6x24", "18x6", "6x6", "24x1", "6x1", "18x1", "6x1"])),
    ((243, 0, LAYER + BIAS), (True, 243, 0xF0, ["24x3", "6x12", "18x3", "6x3", "1x12", "1x3", "1x9", "1x3"])),
    # exactly one round, and one tile more
    ((256, 0, [(128 * 255, 256), (128, 256)]), (True, 256, 0, ["255x1", "1x1"])),
    ((256, 0, [(128 * 255, 256), (128, 257)]), (False, 2 * 255 + 3, 0, ["255x2", "1x3"])),
    ((256, 0, [(1024, 8448)]), (False, 8 * 66, 0, ["8x66"])),   # 264 tiles of 128 x 256
    ((256, 0, [(1024, 8192)]), (True, 256, 0, ["8x32"])),
    # partial tiles and the exchange threshold (N <= 4)
    ((256, 0, [(136, 264)]), (True, 4, 0, ["2x2"])),
    ((256, 0, [(1, 1)]), (True, 1, 1, ["1x1"])),
    ((256, 0, [(520, 4), (520, 5)]), (True, 3 + 5, 1, ["1x3", "5x1"])),
    ((1, 0, [(128, 256)]), (True, 1, 0, ["1x1"])),
    ((1, 0, [(129, 256)]), (False, 4, 0, ["2x2"])),
    # sizes whose tile counts would overflow an int stay in range (the library then rejects the group)
    ((256, 0, [(1 << 40, 1 << 40)]), (False, None, 0, None)),
]


@pytest.fixture(scope="module")
def group_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("group_check") / "group_check")
    subprocess.check_call(["make", "-s", "-C", CSRC, "group_check", f"GROUP_CHECK={exe}"])
    return exe


def test_group_plan_table(group_check):
    lines = "".join(f"{cus} {force} " + " ".join(f"{m} {n}" for m, n in mn) + "\n" for (cus, force, mn), _ in TABLE)
    out = subprocess.run([group_check], input=lines, check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(TABLE)
    for (case, (big, total, swap, tiles)), got in zip(TABLE, out):
        f = got.split()
        assert f[0] == ("big" if big else "small"), (case, got)
        assert int(f[2]) == swap, (case, got)
        if total is None:
            assert int(f[1]) >= 1 << 30, (case, got)
            continue
        assert int(f[1]) == total, (case, got)
        assert f[3:] == tiles, (case, got)
