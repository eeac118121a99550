"""Validation loop (the caller side of greedy decode, src/eval.py:160-229,311-386).

Generates one caption per unique image with ImageCaptioningModel.generate (KV-cached HIP
decode) and writes the reference's predictions JSON ([{"image_id", "caption"}],
eval.py:368-373). COCO metrics (BLEU/ROUGE-L/CIDEr, eval.py:59-108): by default through
pycocoevalcap when it is importable (it is not installed in this image: no metric then);
with `metrics="device"` through icap.metrics.DeviceCaptionMetrics, this package's own
kernels, which need no third-party package.
"""

from __future__ import annotations

import json
import os
from typing import Any, Dict

import torch


def generate_predictions(model, dataset, batch_size: int = 128, max_length: int = 50, temperature: float = 0.0,
                         top_p: float = 0.9, device=None, rat=None):
    """rat: (db_store, top_k, top_i) for a RetrievalAugmentedTransformer (src/eval.py:281-289)."""
    device = device or model.device
    seen, idx = set(), []
    for i in range(len(dataset)):  # one caption per image (eval.py:219-224)
        iid = dataset.captions[i].image_id if hasattr(dataset, "captions") else dataset[i]["image_id"]
        if iid not in seen:
            seen.add(iid)
            idx.append(i)
    preds = []
    for s in range(0, len(idx), batch_size):
        items = [dataset[i] for i in idx[s:s + batch_size]]
        emb = torch.stack([it["image_embedding"] for it in items]).to(device)
        if rat is None:
            ids = model.generate(emb, max_length=max_length, temperature=temperature, top_p=top_p)
        else:
            ids = model.generate(db_store=rat[0], top_k=rat[1], top_i=rat[2], image_embeddings=emb,
                                 max_length=max_length, temperature=temperature, top_p=top_p)
        if hasattr(model.tokenizer, "batch_decode"):
            texts = model.tokenizer.batch_decode(ids.cpu(), skip_special_tokens=True)
        else:
            texts = [" ".join(str(t) for t in row) for row in ids.cpu().tolist()]
        preds += [{"image_id": it["image_id"], "caption": t} for it, t in zip(items, texts)]
    return preds


METRIC_KEYS = ("BLEU-1", "BLEU-2", "BLEU-3", "BLEU-4", "ROUGE-L", "CIDEr")  # EvalMetrics.to_dict, eval.py:39-48


def load_coco_references(annotations_path: str) -> Dict[int, list]:
    """src/eval.py:110-130: image_id -> its reference captions, in annotation order."""
    with open(annotations_path) as f:
        coco = json.load(f)
    refs: Dict[int, list] = {}
    for a in coco["annotations"]:
        refs.setdefault(a["image_id"], []).append(a["caption"])
    return refs


METRIC_BACKENDS = ("pycocoevalcap", "device")


def _check_backend(backend) -> None:
    from .metrics import DeviceCaptionMetrics

    if not isinstance(backend, DeviceCaptionMetrics) and backend not in METRIC_BACKENDS:
        raise ValueError(f'caption metrics backend must be "pycocoevalcap", "device" or a DeviceCaptionMetrics, '
                         f'not {backend!r}')


def compute_caption_metrics(preds, annotations_path: str, backend="pycocoevalcap") -> Dict[str, float]:
    """src/eval.py:59-108,133-157 — BLEU-1..4 / ROUGE-L / CIDEr over the images present in both predictions and
    references (ValueError when none are), keyed as EvalMetrics.to_dict (eval.py:39-48).
    backend "pycocoevalcap" (the default): that package when it is importable, else an empty dict (it is not in this
    image). backend "device": metrics.DeviceCaptionMetrics built from annotations_path, the same numbers counted by
    this package's own kernels; a DeviceCaptionMetrics instance is used as it is (annotations_path is not read)."""
    _check_backend(backend)
    if backend != "pycocoevalcap":
        from .metrics import DeviceCaptionMetrics

        scorer = backend if isinstance(backend, DeviceCaptionMetrics) else DeviceCaptionMetrics(annotations_path)
        return scorer.score(preds)
    try:
        from pycocoevalcap.bleu.bleu import Bleu
        from pycocoevalcap.cider.cider import Cider
        from pycocoevalcap.rouge.rouge import Rouge
    except ImportError:
        return {}
    res_all = {p["image_id"]: [p["caption"]] for p in preds}
    refs_all = load_coco_references(annotations_path)
    common = set(res_all) & set(refs_all)
    if not common:
        raise ValueError("No common image IDs found between predictions and references")
    res = {k: res_all[k] for k in common}
    refs = {k: refs_all[k] for k in common}
    out: Dict[str, float] = {}
    bleu, _ = Bleu(4).compute_score(refs, res)
    for k, v in zip(METRIC_KEYS[:4], bleu):
        out[k] = v
    out["ROUGE-L"], _ = Rouge().compute_score(refs, res)
    out["CIDEr"], _ = Cider().compute_score(refs, res)
    return out


def evaluate_epoch(model, dataset, annotations_path, epoch, split_name, batch_size, num_workers, max_length,
                   temperature, top_p, device, output_dir, *, metrics="pycocoevalcap") -> Dict[str, Any]:
    """src/eval.py:311-386: predictions -> `epoch_{epoch}_{split}_predictions.json` ([{"image_id", "caption"}],
    indent 2) and `epoch_{epoch}_{split}_metrics.json` ({"epoch", "split", "num_images", **metrics}), the
    reference's file names and layouts. Returns the metrics dict (EvalMetrics.to_dict keys). metrics: the backend
    of compute_caption_metrics."""
    model.eval()
    os.makedirs(output_dir, exist_ok=True)
    preds = generate_predictions(model, dataset, batch_size, max_length, temperature, top_p, device)
    m = compute_caption_metrics(preds, annotations_path, backend=metrics) if annotations_path else {}
    with open(os.path.join(output_dir, f"epoch_{epoch}_{split_name}_predictions.json"), "w") as f:
        json.dump(preds, f, indent=2)
    with open(os.path.join(output_dir, f"epoch_{epoch}_{split_name}_metrics.json"), "w") as f:
        json.dump({"epoch": epoch, "split": split_name, "num_images": len(preds), **m}, f, indent=2)
    return m


def generate_and_evaluate_rat(model, db_store, top_k: int, top_i: int, dataset, annotations_path, batch_size: int = 32,
                              num_workers: int = 4, max_length: int = 50, temperature: float = 1.0,
                              top_p: float = 0.9, device=None, *, metrics="pycocoevalcap"):
    """src/eval.py:232-308: (predictions, metrics dict) of a RetrievalAugmentedTransformer over `db_store`. metrics:
    the backend of compute_caption_metrics."""
    model.eval()
    preds = generate_predictions(model, dataset, batch_size, max_length, temperature, top_p, device,
                                 rat=(db_store, top_k, top_i))
    return preds, (compute_caption_metrics(preds, annotations_path, backend=metrics) if annotations_path else {})


def evaluate_rat_epoch(model, db_store, top_k: int, top_i: int, dataset, annotations_path, epoch, split_name,
                       batch_size: int = 32, num_workers: int = 4, max_length: int = 50, temperature: float = 1.0,
                       top_p: float = 0.9, device=None, output_dir: str = "eval_results", *,
                       metrics="pycocoevalcap") -> Dict[str, Any]:
    """src/eval.py:391-476: evaluate_epoch for the retrieval-augmented model; the files carry the reference's
    `_rat` suffix (`epoch_{epoch}_{split}_predictions_rat.json`, `epoch_{epoch}_{split}_metrics_rat.json`)."""
    os.makedirs(output_dir, exist_ok=True)
    preds, m = generate_and_evaluate_rat(model, db_store, top_k, top_i, dataset, annotations_path, batch_size,
                                         num_workers, max_length, temperature, top_p, device, metrics=metrics)
    with open(os.path.join(output_dir, f"epoch_{epoch}_{split_name}_predictions_rat.json"), "w") as f:
        json.dump(preds, f, indent=2)
    with open(os.path.join(output_dir, f"epoch_{epoch}_{split_name}_metrics_rat.json"), "w") as f:
        json.dump({"epoch": epoch, "split": split_name, "num_images": len(preds), **m}, f, indent=2)
    return m


LOSS_KEYS = ("val_loss", "val_perplexity", "val_token_accuracy")


@torch.no_grad()
def evaluate_loss(model, dataset, batch_size: int = 128, num_workers: int = 4, device=None, rat=None,
                  use_graph: bool = True) -> Dict[str, Any]:
    """Teacher-forced validation loss over EVERY caption of `dataset` (not one per image): the reference's loss
    (src/models.py:286-325), i.e. sum of the captions' nll over the number of target tokens, its exponential and the
    share of targets whose label is the argmax of the logits. One engine.CaptionScorer per batch shape (a short last
    batch gets its own), running totals on the device, one host read at the end. rat: (db_store, top_k, top_i) for a
    RetrievalAugmentedTransformer."""
    import math

    from torch.utils.data import DataLoader

    from .engine import CaptionScorer
    from .train import _collate

    device = device or model.device
    was_training = model.training
    model.eval()
    dl = DataLoader(dataset, batch_size=batch_size, shuffle=False, num_workers=num_workers, collate_fn=_collate,
                    pin_memory=True, drop_last=False)
    scorers: Dict[Any, Any] = {}
    totals = torch.zeros(3, dtype=torch.float64, device=device)
    aug_out: Dict[int, torch.Tensor] = {}
    n_caps = 0
    for batch in dl:
        ids, mask, labels, emb = batch["token_ids"], batch["attention_mask"], batch["labels"], batch["image_embedding"]
        B, Lc = ids.shape
        sc = scorers.get((B, Lc))
        if sc is None:
            sc = scorers[(B, Lc)] = CaptionScorer(model, B, Lc)
            sc.totals = totals  # every shape adds to the same running totals
        if rat is not None:
            if B not in aug_out:
                aug_out[B] = torch.empty((B, emb.shape[1]), dtype=torch.float32, device=device)
            emb = model.augment(rat[0], emb.to(device, non_blocking=True), rat[2], rat[1], out=aug_out[B])
        sc.load_batch(ids, mask, labels, emb)
        sc.run(use_graph=use_graph)
        n_caps += B
    t = totals.cpu().tolist()  # the one host read
    model.train(was_training)
    nll, ntok, nhit = t[0], int(round(t[1])), int(round(t[2]))
    loss = nll / ntok if ntok else float("nan")
    try:
        ppl = math.exp(loss)
    except OverflowError:
        ppl = float("inf")
    return {"val_loss": loss, "val_perplexity": ppl, "val_token_accuracy": nhit / ntok if ntok else float("nan"),
            "num_captions": n_caps, "num_tokens": ntok}


def save_eval_summary(all_metrics, output_path: str) -> None:
    """src/eval.py:479-491: the per-epoch validation dicts ({"epoch", "loss", **metrics}) as one JSON list."""
    with open(output_path, "w") as f:
        json.dump(all_metrics, f, indent=2)
    print(f"Evaluation summary saved to: {output_path}")
