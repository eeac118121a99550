"""Time the caption metrics (icap.metrics.DeviceCaptionMetrics) on a synthetic corpus with the geometry of the COCO
val2017 captions: 5 000 images, 5 references each, 8 ... 14 words per caption drawn Zipf-distributed from a
10 000-word vocabulary, one hypothesis per image (a reference of the image with a third of its words redrawn). Seeded.

  device   one pass of icap_caption_metrics, HIP events around each stage (build: table clear + n-gram identity;
           df: document frequencies; score: the per-image kernel), the stages run in order on one workspace
  score    wall time of DeviceCaptionMetrics.score(): host tokenisation and packing of the hypotheses, the upload,
           the pass, the one read-back, the host finishing; its host packing share is timed separately
  python   wall time of the plain-Python restatement (tests/caption_metric_refs.py) on the same corpus and machine.
           pycocoevalcap is not installed here: the restatement does the same dictionary work in the same way and is
           its STAND-IN, not the package itself. It is single-threaded however many cores are free.

Medians over `--rounds` after a warm-up. The scores of the two routes are compared on the way.

Run:  python tools/caption_metrics_bench.py [--out profiles/caption_metrics_bench.json]
Prints one JSON line. Not a test: no threshold."""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpt2-image-captioning_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import caption_metric_refs as R  # noqa: E402
from icap import _lib, ops  # noqa: E402
from icap.metrics import DeviceCaptionMetrics  # noqa: E402


def corpus(images: int, refs: int, vocab: int, seed: int):
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, vocab + 1)
    p /= p.sum()
    words = [f"w{i}" for i in range(vocab)]
    pool = iter(rng.choice(vocab, size=images * (refs + 1) * 14, p=p).tolist())  # every word drawn, in one call

    def caption():
        return [words[next(pool)] for _ in range(int(rng.integers(8, 15)))]

    gts, res = {}, {}
    for i in range(images):
        rs = [caption() for _ in range(refs)]
        h = list(rs[int(rng.integers(0, refs))])
        for j in range(len(h)):
            if rng.random() < 1 / 3:
                h[j] = words[next(pool)]
        gts[i] = [" ".join(r) for r in rs]
        res[i] = " ".join(h)
    return gts, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--refs", type=int, default=5)
    ap.add_argument("--vocab", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--python-rounds", type=int, default=1, help="runs of the plain-Python restatement")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("caption_metrics_bench: no GPU (timings come from the device only)")
    dev = torch.device("cuda", 0)
    gts, res = corpus(a.images, a.refs, a.vocab, a.seed)
    preds = [{"image_id": i, "caption": c} for i, c in res.items()]

    t0 = time.perf_counter()
    sc = DeviceCaptionMetrics(gts, device=dev)
    torch.cuda.synchronize()
    build_scorer_s = time.perf_counter() - t0

    # the stages alone, on one workspace, events between them
    batch = sc.pack(preds)
    caps = ops.caption_metrics_capacities(batch.positions)
    ws = sc.workspace(batch, caps)
    stages = (("build", _lib.METRIC_STAGE_BUILD), ("df", _lib.METRIC_STAGE_DF), ("score", _lib.METRIC_STAGE_SCORE))
    ms = {k: [] for k, _ in stages}
    ms["pass"] = []
    for r in range(a.warmup + a.rounds):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        for n, (_, bit) in enumerate(stages):
            ops.caption_metrics(batch.arrays, **batch.kwargs(caps, ws, stages=bit))
            ev[n + 1].record()
        ev[3].synchronize()
        if r >= a.warmup:
            for n, (k, _) in enumerate(stages):
                ms[k].append(ev[n].elapsed_time(ev[n + 1]))
            ms["pass"].append(ev[0].elapsed_time(ev[3]))
    staged = batch.read()

    wall, pack = [], []
    out = None
    for r in range(a.warmup + a.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = sc.score(preds)
        t1 = time.perf_counter()
        sc.pack(preds)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if r >= a.warmup:
            wall.append((t1 - t0) * 1e3)
            pack.append((t2 - t1) * 1e3)
    assert abs(float(np.mean(staged[2])) - out["CIDEr"]) == 0.0  # the staged pass and score() agree bitwise

    py = []
    want = None
    for _ in range(a.python_rounds):
        t0 = time.perf_counter()
        want = R.score(gts, res)
        py.append(time.perf_counter() - t0)
    diff = {k: abs(out[k] - want["metrics"][k]) for k in R.KEYS}

    med = {k: statistics.median(v) for k, v in ms.items()}
    result = {
        "corpus": {"images": a.images, "references_per_image": a.refs, "words_per_caption": "8..14",
                   "vocabulary": a.vocab, "distribution": "zipf (1/rank)", "seed": a.seed,
                   "ngram_positions_orders_2_3_4": list(batch.positions), "table_capacities": list(caps),
                   "workspace_MiB": round(ws.numel() / 2 ** 20, 2)},
        "rounds": a.rounds, "warmup": a.warmup,
        "device_ms": {k: round(v, 4) for k, v in med.items()},
        "device_ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
        "score_wall_ms": round(statistics.median(wall), 3),
        "score_wall_ms_min_max": [round(min(wall), 3), round(max(wall), 3)],
        "host_pack_and_upload_ms": round(statistics.median(pack), 3),
        "scorer_construction_s": round(build_scorer_s, 3),
        "python_restatement_s": round(statistics.median(py), 3),
        "python_restatement_is": "tests/caption_metric_refs.py, a stand-in for pycocoevalcap (not installed)",
        "speedup_wall_vs_python": round(statistics.median(py) * 1e3 / statistics.median(wall), 1),
        "metrics": {k: out[k] for k in R.KEYS},
        "abs_diff_vs_python": diff,
        "device": torch.cuda.get_device_name(0),
    }
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
