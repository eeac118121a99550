"""CLIP extraction with host decode against device decode (icap.images.extract_directory(device_decode=...)), in one
session on one GPU: N synthetic 480 x 640 q90 4:2:0 JPEGs (gradient + noise, sized like COCO files) through
extract_clip_embeddings' loop at 4 / 8 / 16 workers and batch 32 / 256, each leg warmed once and timed REPS times,
host and device decode alternating. Then, in a run of their own, icap_jpeg_decode's three kernels per batch between
HIP events. The host-decode legs are the default path and the baseline. Writes profiles/jpeg_extract_bench.json
(--out) and prints it.

    python tools/jpeg_extract_bench.py [--images 2048] [--reps 2] [--out profiles/jpeg_extract_bench.json]
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gpt2-image-captioning_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

from icap import _lib, jpeg, ops  # noqa: E402
from icap.clip import CLIPVisionTower, DeviceCLIPProcessor  # noqa: E402
from icap.images import extract_directory  # noqa: E402


def write_images(d: str, n: int) -> int:
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:480, 0:640]
    total = 0
    for i in range(n):
        base = np.stack([(xx * (1 + i % 5) + yy * (i % 3)) % 256, (yy * 2 + i * 7) % 256,
                         (xx + yy + i * 13) % 256], -1).astype(np.int16)
        img = np.clip(base + rng.integers(-40, 40, base.shape), 0, 255).astype(np.uint8)
        path = os.path.join(d, f"COCO_val2014_{i:012d}.jpg")
        Image.fromarray(img).save(path, quality=90, subsampling="4:2:0")
        total += os.path.getsize(path)
    return total


def kernel_times(d: str, dev, batch: int, reps: int = 10) -> dict:
    """Median ms of each icap_jpeg_decode stage over one batch of files already on the device."""
    names = sorted(os.listdir(d))[:batch]
    items = []
    for nm in names:
        data = open(os.path.join(d, nm), "rb").read()
        items.append((data, jpeg.parse_jpeg(data)))
    b = jpeg.pack_batch(items)
    toc = b.toc.tolist()
    blob = b.blob.to(dev)
    blocks = toc[jpeg.TOC_TOTAL_BLOCKS]
    coef = torch.empty(blocks * 64, dtype=torch.int16, device=dev)
    planes = torch.empty(blocks * 64, dtype=torch.uint8, device=dev)
    out = torch.empty(toc[jpeg.TOC_OUT_BYTES], dtype=torch.uint8, device=dev)
    status = torch.empty(len(items), dtype=torch.int32, device=dev)
    stages = [("entropy", _lib.JPEG_STAGE_ENTROPY), ("idct", _lib.JPEG_STAGE_IDCT), ("colour", _lib.JPEG_STAGE_COLOUR),
              ("all", _lib.JPEG_STAGE_ALL)]
    for _ in range(2):  # warm-up: code object, caches
        ops.jpeg_decode(toc, blob, coef, planes, out, status)
    torch.cuda.synchronize(dev)
    res = {}
    for name, mask in stages:
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.jpeg_decode(toc, blob, coef, planes, out, status, stages=mask)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        res[f"{name}_ms"] = round(statistics.median(ms), 4)
        res[f"{name}_ms_min_max"] = [round(min(ms), 4), round(max(ms), 4)]
    assert status.cpu().tolist() == [0] * len(items)
    res.update(batch=len(items), compressed_bytes=int(toc[jpeg.TOC_DATA_BYTES]), blocks=int(blocks),
               images_per_s_all=round(len(items) / (res["all_ms"] / 1e3), 1))
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--workers", type=int, nargs="+", default=[4, 8, 16])
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 256])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_extract_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    _lib.require_device(dev)
    tower = CLIPVisionTower.random_init(seed=0).to(dev)
    proc = DeviceCLIPProcessor(device=dev)
    dim = tower.config.projection_dim
    d = tempfile.mkdtemp(prefix="icap_jpeg_bench_")
    res = {"images": a.images, "image": "480x640 JPEG q90 4:2:0, gradient + noise", "reps": a.reps,
           "device": torch.cuda.get_device_name(dev), "legs": []}
    try:
        res["mean_file_bytes"] = round(write_images(d, a.images) / a.images)
        out = os.path.join(d, "emb.pt")
        for batch in a.batches:
            for workers in a.workers:
                runs = {False: [], True: []}
                stats = {}
                for mode in (False, True):  # warm-up of both paths: page cache, kernels, allocator
                    extract_directory(d, out, tower.embed, proc, dim, batch, workers, dev, device_decode=mode)
                torch.cuda.synchronize(dev)
                for _ in range(a.reps):
                    for mode in (False, True):  # alternating
                        st = {}
                        t0 = time.perf_counter()
                        n = extract_directory(d, out, tower.embed, proc, dim, batch, workers, dev, stats=st,
                                              device_decode=mode)
                        torch.cuda.synchronize(dev)
                        runs[mode].append(n / (time.perf_counter() - t0))
                        stats[mode] = st
                leg = {"batch": batch, "workers": workers}
                for mode, key in ((False, "host_decode"), (True, "device_decode")):
                    leg[key] = {"images_per_s": round(statistics.median(runs[mode]), 1),
                                "images_per_s_runs": [round(r, 1) for r in runs[mode]],
                                "main_process_split_s": stats[mode]}
                leg["device_over_host"] = round(leg["device_decode"]["images_per_s"] /
                                                leg["host_decode"]["images_per_s"], 3)
                res["legs"].append(leg)
                print(json.dumps(leg), flush=True)
        res["kernels"] = [kernel_times(d, dev, b) for b in a.batches]
    finally:
        shutil.rmtree(d, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
