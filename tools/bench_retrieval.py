"""Time RetrievalAugmentedTransformer.augment at COCO-train size against the reference-shaped host path.

Device path: the score GEMM, icap_topk_rows and icap_retrieval_aggregate captured in one graph; the time is HIP
events around `--iters` replays (after warm-up), per replay. Host path, on the same machine: what the reference does
per forward (src/models.py:675-695) with numpy's exact search in place of FAISS: queries to the host, S = Q . X^T,
top_i + 10 per row, the filter and the filename -> caption-rows walk, one row copy per caption, the result back to
the device; wall clock ending in a device synchronise.

Run:  python tools/bench_retrieval.py [--out profiles/retrieval_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, "gpt2-image-captioning_amd"))

from icap import DeviceRetrievalStore, ops  # noqa: E402


def unit_rows(n, d, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn((n, d), generator=g, device=dev), dim=1)


def host_path(q_dev, images, captions, names, by_name, top_i, top_k, dev):
    q = q_dev.cpu().numpy().astype("float32")
    s = q @ images.T
    K = top_i + 10
    part = np.argpartition(-s, K, axis=1)[:, :K]
    order = np.take_along_axis(part, np.argsort(-np.take_along_axis(s, part, 1), axis=1, kind="stable"), 1)
    out = np.zeros((q.shape[0], top_k, q.shape[1]), dtype=np.float32)
    for b in range(q.shape[0]):
        kept = []
        for i in order[b]:
            if float(s[b, i]) > 0.9999:
                continue
            kept.append(names[i])
            if len(kept) >= top_i:
                break
        rows = []
        for f in kept:
            if f in by_name:
                rows.extend(by_name[f])
                if len(rows) >= top_k:
                    break
        for j, r in enumerate(rows[:top_k]):
            out[b, j] = captions[r]
    r = torch.from_numpy(out).to(dev)
    return q_dev + r.mean(dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=118287)
    ap.add_argument("--captions", type=int, default=591753)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--top-i", type=int, default=4)
    ap.add_argument("--top-k", type=int, default=10)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--host-iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_retrieval: no GPU (timings come from the device only)")
    dev = torch.device("cuda", 0)
    N, C, D, B = a.images, a.captions, a.dim, a.batch
    images, captions = unit_rows(N, D, dev, 0), unit_rows(C, D, dev, 1)
    names = [f"{n:012d}.jpg" for n in range(N)]
    owner = torch.randint(0, N, (C,), generator=torch.Generator().manual_seed(2)).tolist()
    meta = [{"filename": names[n], "caption_id": c} for c, n in enumerate(owner)]
    store = DeviceRetrievalStore(images, captions, names, meta, dev)
    # queries: half database rows (the training case: the self match is filtered), half fresh vectors
    q = torch.cat([images[: B // 2], unit_rows(B - B // 2, D, dev, 3)]).contiguous()
    out = torch.empty((B, D), dtype=torch.float32, device=dev)
    for _ in range(3):
        eager = store.augment(q, a.top_i, a.top_k, "mean", out=out).clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with ops.graph_capture(g):
        store.augment(q, a.top_i, a.top_k, "mean", out=out)
    for _ in range(10):
        g.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    device_ms = e0.elapsed_time(e1) / a.iters
    assert torch.equal(out, eager)

    images_h, captions_h = images.cpu().numpy(), captions.cpu().numpy()
    by_name = {}
    for c, n in enumerate(owner):
        by_name.setdefault(names[n], []).append(c)
    ref = host_path(q, images_h, captions_h, names, by_name, a.top_i, a.top_k, dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.host_iters):
        ref = host_path(q, images_h, captions_h, names, by_name, a.top_i, a.top_k, dev)
    torch.cuda.synchronize()
    host_ms = (time.perf_counter() - t0) * 1e3 / a.host_iters
    res = {"bench": "retrieval_augment", "images": N, "captions": C, "dim": D, "batch": B, "top_i": a.top_i,
           "top_k": a.top_k, "device_graph_ms": round(device_ms, 4), "host_path_ms": round(host_ms, 2),
           "score_bytes": 4 * B * N, "max_abs_diff_vs_host": float((ref - eager).abs().max()),
           "threads": torch.get_num_threads()}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
