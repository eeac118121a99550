"""bench.py as a plain run (GPU): --steps sets the timed steps, the JSON line carries the headline fields and
ms_per_step and none of the --full legs, and --dump-outputs writes the last timed step's loss / parameters /
gradients as float32 .npy files (at most 64 MB in all)."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(dev, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--batch", "8", "--dump-outputs", str(out)], capture_output=True, text=True, env=env,
                       timeout=110)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1
    assert d["unit"] == "images/s" and d["higher_is_better"] is True and d["dtype"] == "bf16"
    assert d["ms_per_step"] > 0
    # value is the images/s of those timed steps (both rounded in the line)
    assert d["value"] == pytest.approx(8 * 1e3 / d["ms_per_step"], rel=1e-3)
    for leg in ("roofline", "greedy_captions_per_s", "batch_sweep", "train_unfrozen", "fp32_parity_mode",
                "clip_extraction", "padded_images_per_s"):
        assert d[leg] is None, leg
    assert "cpu_baseline" not in d
    arrs = {n: np.load(out / f"{n}.npy") for n in ("loss", "params", "grads")}
    assert sorted(os.listdir(out)) == ["grads.npy", "loss.npy", "params.npy"]
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
    for n, a in arrs.items():
        assert a.dtype == np.float32 and np.isfinite(a).all(), n
    assert arrs["loss"].shape == (1,) and float(arrs["loss"][0]) == pytest.approx(d["final_loss"], abs=1e-4)
    assert arrs["params"].shape == arrs["grads"].shape and arrs["params"].size > 1 << 20
    assert np.count_nonzero(arrs["grads"]) > arrs["grads"].size // 2
