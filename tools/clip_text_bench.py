"""Time the CLIP text tower's device schedule (icap.clip_text.ClipTextCore) against the torch restatement on the host.

One process, one shape: the ViT-B/32 text geometry in bf16, 256 captions of 10 ... 22 tokens from the tests' stub
tokenizer, padded to the batch maximum — one chunk of the schedule, under ROWS_CAP, so it launches no GEMM plan that
tests/test_clip_text_gpu.py has not run. Device: (a) eager, the public `get_text_features` call with device ids
(launches + the 4-byte count read-back), host clock around `--iters` calls ending in a device synchronise; (b) graph,
`core.run` captured once, HIP events around `--iters` replays. Both after warm-up. Host: the same captions through
tests/clip_text_helpers.py::text_features_ref (fp32, caption by caption, unpadded) on 16 threads, wall clock of one
pass after a short warm-up. Reports captions/s for each and the parity of the device result with the host's.

Run:  python tools/clip_text_bench.py [--out profiles/clip_text_bench.json]
Prints one JSON line. Not a test: no threshold."""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gpt2-image-captioning_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import clip_text_helpers as H  # noqa: E402
from icap import CLIPTextConfig, CLIPTextTower, ops  # noqa: E402
from icap.clip_text import ROWS_CAP, chunk_captions  # noqa: E402

WORDS = ("a an the man woman dog cat table window kitchen street bus train plate of food with on in standing sitting "
         "next to large small red blue green white black two people holding umbrella park bench grass field").split()


def captions(n: int, seed: int = 0):
    rng = np.random.RandomState(seed)
    return [" ".join(rng.choice(WORDS, size=rng.randint(8, 21))) for _ in range(n)]  # + BOS / EOT: 10 ... 22 tokens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--captions", type=int, default=256)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_text_bench: no GPU (timings come from the device only)")
    dev = torch.device("cuda", 0)
    cfg = CLIPTextConfig()
    tower = CLIPTextTower.random_init(cfg, seed=0)
    sd = {k: v.clone() for k, v in tower.state_dict().items()}
    tower = tower.to(dev)
    ids = H.StubTokenizer(cfg.vocab_size)(text=captions(a.captions))["input_ids"]
    B, L_ = ids.shape
    lens = (ids != 0).sum(1)
    if len(chunk_captions(B, L_)) != 1 or B * L_ > ROWS_CAP:
        raise SystemExit("clip_text_bench: the shape must be one chunk under ROWS_CAP")
    dids = ids.to(dev)
    dt = torch.bfloat16

    for _ in range(a.warmup):
        eager = tower.get_text_features(dids, compute_dtype=dt)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.iters):
        eager = tower.get_text_features(dids, compute_dtype=dt)
    torch.cuda.synchronize()
    eager_ms = (time.perf_counter() - t0) * 1e3 / a.iters

    core = tower.core(dt)
    ws = core.alloc(B, L_)
    ws.ids.copy_(dids)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with ops.graph_capture(g):
        core.run(ws, ws.ids)
    for _ in range(a.warmup):
        g.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    graph_ms = e0.elapsed_time(e1) / a.iters
    same = bool(torch.equal(ws.feat32, eager))

    torch.set_num_threads(a.threads)
    H.text_features_ref(sd, cfg, ids[:8].numpy())
    t0 = time.perf_counter()
    ref = H.text_features_ref(sd, cfg, ids.numpy())
    host_s = time.perf_counter() - t0
    cos = torch.nn.functional.cosine_similarity(eager.double().cpu(), ref.double(), dim=-1)

    res = {"bench": "clip_text_tower", "geometry": "ViT-B/32 text", "dtype": "bf16", "captions": B, "L": L_,
           "tokens_min": int(lens.min()), "tokens_max": int(lens.max()), "token_rows": B * L_, "iters": a.iters,
           "device_eager_ms": round(eager_ms, 4), "device_eager_captions_per_s": round(B / eager_ms * 1e3, 1),
           "device_graph_ms": round(graph_ms, 4), "device_graph_captions_per_s": round(B / graph_ms * 1e3, 1),
           "graph_equals_eager": same, "host_restatement_s": round(host_s, 3),
           "host_captions_per_s": round(B / host_s, 1), "host_threads": torch.get_num_threads(),
           "min_cosine_vs_host_fp32": round(float(cos.min()), 6)}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
