"""Time caption scoring (engine.CaptionScorer) against the only other route to a held-out loss, and against the train
step, in one process at one shape: GPT-2 small + the transformer mapper (random weights), bf16, B = 128 captions of
Lc = 50 slots with 10 ... 22 real tokens each, image embeddings given.

  scorer   graph replays of CaptionScorer.run, HIP events around each block of replays
  forward  `model(ids, emb, mask, labels).loss` under no_grad with one .item() per batch (the full-width LM head on the
           padded [B, P + Lc] grid, fp32 logits, eager): host clock around each block, ending in the .item()
  step     graph replays of CaptionTrainer.micro_step (forward + backward + AdamW) on the same batch, HIP events

The three are timed in alternating blocks (`--rounds` rounds) after a warm-up, so a drift of the clocks falls on all
of them alike; the medians of the blocks are reported. The expectation is an inequality: the scorer runs a subset of the
step's launches (the same forward, no backward, no optimizer), so its time per batch lies below the step's.

Run:  python tools/score_bench.py [--out profiles/score_bench.json]
Prints one JSON line. Not a test: no threshold."""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpt2-image-captioning_amd"))

from icap import (CaptionScorer, CaptionTrainer, GPT2LMHeadModel, ImageCaptioningModel,  # noqa: E402
                  TransformerMappingNetwork)


def synthetic(B: int, Lc: int, seed: int):
    """ids / mask / labels (pinned host tensors, as the loaders deliver them) with 10 ... 22 real tokens per caption,
    the last of them EOS; unit-norm embeddings."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, 50256, (B, Lc), generator=g)
    n = torch.randint(10, 23, (B,), generator=g)
    pos = torch.arange(Lc)[None, :]
    mask = (pos < n[:, None]).long()
    ids[pos >= (n - 1)[:, None]] = 50256
    labels = ids.clone()
    labels[mask == 0] = -100
    emb = torch.randn((B, 512), generator=g)
    emb = emb / emb.norm(dim=-1, keepdim=True)
    return ids.pin_memory(), mask.pin_memory(), labels.pin_memory(), emb.pin_memory()


def event_block(fn, n: int) -> float:
    """ms per call of n back-to-back calls, by HIP events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--caption-len", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replays", type=int, default=50, help="scorer / step replays per block")
    ap.add_argument("--forwards", type=int, default=5, help="forward().loss.item() calls per block")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("score_bench: no GPU (timings come from the device only)")
    dev = torch.device("cuda", 0)
    B, Lc = a.batch, a.caption_len
    gpt = GPT2LMHeadModel.random_init(seed=0)
    mapper = TransformerMappingNetwork.random_init(seed=0)
    model = ImageCaptioningModel(mapper, tokenizer=SimpleNamespace(eos_token_id=50256), gpt=gpt,
                                 compute_dtype=torch.bfloat16).to(dev)
    ids, mask, labels, emb = synthetic(B, Lc, 1)
    scorer = CaptionScorer(model, B, Lc)
    trainer = CaptionTrainer(model, B, Lc, lr=1e-6, num_training_steps=10 ** 6, dropout=True, seed=1234)
    scorer.load_batch(ids, mask, labels, emb)
    trainer.load_batch(ids, mask, labels, emb=emb)
    d = [t.to(dev) for t in (ids, emb, mask, labels)]

    def forward_loss() -> float:
        with torch.no_grad():
            return model(*d).loss.item()

    model.eval()
    for _ in range(a.warmup):
        scorer.run(use_graph=True)
        trainer.micro_step(use_graph=True)
    fwd_loss = forward_loss()
    torch.cuda.synchronize()
    scorer.reset()
    scorer.run(use_graph=True)
    t = scorer.totals.cpu()
    score_loss = float(t[0] / t[1])
    ms = {"scorer": [], "forward": [], "step": []}
    for _ in range(a.rounds):
        ms["scorer"].append(event_block(lambda: scorer.run(use_graph=True), a.replays))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.forwards):
            forward_loss()
        ms["forward"].append((time.perf_counter() - t0) * 1e3 / a.forwards)
        ms["step"].append(event_block(lambda: trainer.micro_step(use_graph=True), a.replays))
    torch.cuda.synchronize()
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = {
        "shape": {"B": B, "Lc": Lc, "P": model.total_prefix_length, "dtype": "bf16", "gpt": "gpt2-small",
                  "mapper": "transformer", "real_tokens": "10..22", "targets": int(t[1])},
        "rounds": a.rounds, "replays_per_block": a.replays, "forwards_per_block": a.forwards,
        "scorer_ms_per_batch": round(med["scorer"], 4), "scorer_captions_per_s": round(B / med["scorer"] * 1e3, 1),
        "forward_item_ms_per_batch": round(med["forward"], 4),
        "forward_item_captions_per_s": round(B / med["forward"] * 1e3, 1),
        "train_step_ms": round(med["step"], 4),
        "scorer_below_step": bool(med["scorer"] < med["step"]),
        "blocks_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
        "loss_scorer": score_loss, "loss_forward": fwd_loss,
        "device": torch.cuda.get_device_name(0),
    }
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
