"""Caption metrics on the device (icap.metrics.DeviceCaptionMetrics, csrc/caption_metrics.hip) against the
plain-Python restatement (tests/caption_metric_refs.py).

Bounds (from the issue, none from the code under test): BLEU's stats rows and the LCS lengths are integers and must
be equal; BLEU and ROUGE-L, per image and over the corpus, then follow from the same fp64 arithmetic within 1e-12
relative (a few ulps of ** and exp). CIDEr per image is an fp64 sum of at most 4 x 128 non-negative products in
another order (about 1e-13 on the 0..10 scale): 1e-10 absolute, and the same for the corpus mean. Two calls on the
same input are bitwise equal in every output."""

import functools
import glob
import json
import os

import numpy as np
import pytest
import torch

import caption_metric_refs as R
from icap import metrics as M
from icap import ops
from test_caption_metrics_cpu import ANCHOR, ANCHOR_REFS, ANCHOR_RES, random_corpus

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "caption_preds_sample.json")


def _flat(pairs):
    return [v for ls in pairs for v in ls]


def _check_integers(want, ids, stats, lcs):
    assert list(ids) == want["ids"]
    bad = [(i, s, w) for i, s, w in zip(ids, stats.tolist(), want["stats"]) if s != w]
    assert not bad, bad[:5]
    assert lcs.tolist() == _flat(want["lcs"])


def _check_floats(want, out):
    errs = {"bleu_rouge_rel": 0.0, "cider_abs": 0.0}

    def rel(a, b, what):
        e = abs(a - b) / abs(b) if b != 0 else abs(a)
        errs["bleu_rouge_rel"] = max(errs["bleu_rouge_rel"], e)
        return e <= 1e-12, (what, a, b)

    def cid(a, b, what):
        errs["cider_abs"] = max(errs["cider_abs"], abs(a - b))
        return abs(a - b) <= 1e-10, (what, a, b)

    checks = []
    for k in R.KEYS:
        f = cid if k == "CIDEr" else rel
        checks.append(f(out[k], want["metrics"][k], k))
        for i in want["ids"]:
            checks.append(f(out["per_image"][i][k], want["per_image"][i][k], (i, k)))
    print("largest errors:", errs)
    for ok, what in checks:
        assert ok, what
    assert set(out["per_image"]) == set(want["ids"])


def _compare(dev, gts, res):
    """Score `res` against `gts` on the device and by the restatement; integers equal, floats within the bounds."""
    sc = M.DeviceCaptionMetrics(gts, device=dev)
    want = R.score(gts, res)
    ids, stats, lcs, cider, _ = sc.device_pass(res)
    _check_integers(want, ids, stats, lcs)
    out = sc.score(res, per_image=True)
    _check_floats(want, out)
    assert all(isinstance(out[k], float) for k in R.KEYS)
    return want, out, stats


def test_anchor(dev):
    preds = [{"image_id": i, "caption": c} for i, c in ANCHOR_RES.items()]
    out = M.DeviceCaptionMetrics(ANCHOR_REFS, device=dev).score(preds)
    print(out)
    for k in R.KEYS[:5]:
        assert abs(out[k] - ANCHOR[k]) <= 1e-12 * ANCHOR[k], (k, out[k], ANCHOR[k])
    assert abs(out["CIDEr"] - ANCHOR["CIDEr"]) <= 1e-10
    _compare(dev, ANCHOR_REFS, ANCHOR_RES)


W128 = " ".join(f"t{i % 37}" for i in range(128))
EDGE = {
    "empty_hypothesis": ({1: ["a cat on a mat", "the cat"], 2: ["two dogs run"]}, {1: "", 2: "two dogs"}),
    "short_hypotheses": ({1: ["a cat on a mat"], 2: ["a cat sat"], 3: ["the dog runs far away"]},
                         {1: "cat", 2: "a cat", 3: "the dog runs"}),
    "one_image": ({7: ["a cat on a mat", "a cat"]}, {7: "a cat on the mat"}),
    "ngram_in_every_image": ({1: ["a cat sits", "big a cat"], 2: ["a cat runs"], 3: ["see a cat"]},
                             {1: "a cat", 2: "a cat runs off", 3: "a dog"}),
    "unseen_ngram_twice": ({1: ["a cat on a mat"], 2: ["two dogs run"]}, {1: "zz yy zz yy a cat", 2: "two qq qq"}),
    "closest_length_tie": ({1: ["a b c d e f", "a b c d"], 2: ["x y", "x y z w"]}, {1: "a b c d e", 2: "x y z"}),
    "spaces": ({1: ["a cat  on the mat ", " a cat"], 2: ["two dogs\n", "two  dogs run "]},
               {1: "a  cat on the mat", 2: "two dogs "}),
    "one_and_seven_references": ({1: ["a cat"], 2: ["a dog", "the dog", "a dog runs", "dog", "a a dog", "big dog",
                                                    "a dog a dog"]}, {1: "a cat sat", 2: "a dog a dog"}),
    "exactly_128_tokens": ({1: [W128, W128 + "\n"], 2: [" ".join(reversed(W128.split())), "t1 t2"]},
                           {1: " ".join(reversed(W128.split())), 2: W128}),
}


@pytest.mark.parametrize("name", list(EDGE))
def test_edge_case(dev, name):
    gts, res = EDGE[name]
    want, out, stats = _compare(dev, gts, res)
    if name == "empty_hypothesis":
        assert stats[0].tolist()[:6] == [0, 2, 0, 0, 0, 0]
    if name == "short_hypotheses":
        assert stats[:, 2:6].tolist() == [[1, 0, 0, 0], [2, 1, 0, 0], [3, 2, 1, 0]]
    if name == "one_image":
        assert out["CIDEr"] == 0.0
    if name == "closest_length_tie":
        assert stats[:, 1].tolist() == [4, 2]
    if name == "exactly_128_tokens":
        assert stats[:, 0].tolist() == [128, 128]


@functools.lru_cache(maxsize=None)
def _corpus(kind):
    gts, res = random_corpus(11, vocab=12) if kind == "a" else random_corpus(12, vocab=5000)
    return gts, res, R.score(gts, res)


@pytest.mark.parametrize("kind", ["a", "b"])
def test_random_corpus(dev, kind):
    gts, res, want = _corpus(kind)
    assert len(want["ids"]) == 64
    sc = M.DeviceCaptionMetrics(gts, device=dev)
    ids, stats, lcs, cider, _ = sc.device_pass(res)
    _check_integers(want, ids, stats, lcs)
    out = sc.score(res, per_image=True)
    _check_floats(want, out)
    # two calls on the same input: every output bitwise equal
    ids2, stats2, lcs2, cider2, _ = sc.device_pass(res)
    assert ids2 == ids and np.array_equal(stats, stats2) and np.array_equal(lcs, lcs2)
    assert np.array_equal(cider.view(np.int64), cider2.view(np.int64))
    out2 = sc.score(res, per_image=True)
    assert out2 == out


def test_random_corpus_smallest_capacities(dev):
    """Corpus (a) through ops.caption_metrics with the smallest capacities the library accepts: the tables run
    nearly full, so the probe chains are long."""
    gts, res, want = _corpus("a")
    sc = M.DeviceCaptionMetrics(gts, device=dev)
    batch = sc.pack(res)
    caps = tuple(1 << int(n).bit_length() for n in batch.positions)  # the next power of two > positions
    assert all(c > p and c <= 2 * max(p, 1) for c, p in zip(caps, batch.positions))
    ws = torch.empty(ops.caption_metrics_workspace(batch.n_vocab, batch.n_ref_words, batch.n_hyp_words, caps),
                     dtype=torch.uint8, device=dev)
    ops.caption_metrics(batch.arrays, **batch.kwargs(caps, ws))
    stats, lcs, cider = batch.read()
    _check_integers(want, batch.ids, stats, lcs)
    err = max(abs(c - want["per_image"][i]["CIDEr"]) for c, i in zip(cider.tolist(), batch.ids))
    print("largest per-image CIDEr error:", err)
    assert err <= 1e-10
    assert abs(float(np.mean(cider)) - want["metrics"]["CIDEr"]) <= 1e-10


def test_subset_scoring(dev):
    """20 of the 64 images and 3 ids the references do not hold: N and the document frequencies follow the 20."""
    gts, res, full = _corpus("a")
    keep = sorted(res)[5:64:3][:20]
    sub = {i: res[i] for i in keep}
    preds = [{"image_id": i, "caption": c} for i, c in sub.items()]
    preds += [{"image_id": 5, "caption": "w1 w2"}, {"image_id": 6, "caption": "w" * 3 + " x" * 200},
              {"image_id": 10 ** 6, "caption": ""}]  # dropped unpacked: 201 words are no error here
    want = R.score(gts, sub)
    assert len(want["ids"]) == 20
    sc = M.DeviceCaptionMetrics(gts, device=dev)
    ids, stats, lcs, cider, _ = sc.device_pass(preds)
    _check_integers(want, ids, stats, lcs)
    _check_floats(want, sc.score(preds, per_image=True))
    assert want["metrics"]["CIDEr"] != full["metrics"]["CIDEr"]
    with pytest.raises(ValueError, match="No common image IDs"):
        sc.score(preds[-3:])
    with pytest.raises(ValueError, match=f"image {keep[0]}"):
        sc.score([{"image_id": keep[0], "caption": "x " * 200}])


def test_realistic_text(dev):
    """Generated captions of the reference (tokens such as `field!!!!!!!!!!!!!!!`) as hypotheses; references derived
    from them: a word dropped, neighbouring words swapped, the neighbouring entry's caption."""
    entries = json.load(open(GOLDEN))
    assert len(entries) == 200
    caps = [e["caption"] for e in entries]
    gts = {}
    for n, e in enumerate(entries):
        w = caps[n].split()
        dropped = " ".join(x for j, x in enumerate(w) if j % 3 != 1)
        swapped = list(w)
        for j in range(0, len(swapped) - 1, 2):
            swapped[j], swapped[j + 1] = swapped[j + 1], swapped[j]
        refs = [dropped, " ".join(swapped) + " ", caps[(n + 1) % len(caps)]]
        gts.setdefault(e["image_id"], []).extend(refs[:1 + n % 3])
    _compare(dev, gts, {e["image_id"]: e["caption"] for e in entries})
    sc = M.DeviceCaptionMetrics(gts, device=dev)
    assert sc.score(entries) == sc.score({e["image_id"]: [e["caption"]] for e in entries})  # list or dict of lists


def test_train_selects_by_device_cider(dev, tmp_path):
    import icap
    from icap.dataset import SyntheticCaptionDataset
    from icap.evaluate import METRIC_KEYS, evaluate_epoch
    from test_score_gpu import TINY_G, TINY_M, build

    tr = SyntheticCaptionDataset(8, max_length=12, real=5, vocab_size=512, eos=511, embed_dim=64)
    va = SyntheticCaptionDataset(6, max_length=12, real=5, vocab_size=512, eos=511, embed_dim=64, seed=2)
    # the tiny model has no tokenizer: its captions are the token numbers; references of token numbers overlap them
    ann = {"annotations": [{"image_id": i, "caption": " ".join(str(t) for t in range(r, 512, 4))}
                           for i in range(6) for r in range(1 + i % 3)]}
    ann_path = tmp_path / "annotations.json"
    ann_path.write_text(json.dumps(ann))
    model = build(TINY_G, TINY_M, torch.float32, dev)
    out = icap.train(tr, model, batch_size=4, num_epochs=2, num_workers=0, learning_rate=1e-3, device=dev,
                     outputs_dir=str(tmp_path), save_every_epoch=10, val_dataset=va,
                     val_annotations_path=str(ann_path), eval_batch_size=4, eval_max_length=4, dropout=False,
                     caption_metrics="device")
    vm = out["val_metrics"]
    assert len(vm) == 2
    for m in vm:
        assert set(METRIC_KEYS) <= set(m) and all(np.isfinite(m[k]) for k in METRIC_KEYS)
    ciders = [m["CIDEr"] for m in vm]
    assert out["best_val_cider"] == max(ciders)
    assert out["best_epoch"] == 1 + ciders.index(max(ciders))
    best = [os.path.basename(p) for p in glob.glob(os.path.join(tmp_path, "best_model_epoch_*.pt"))]
    assert f"best_model_epoch_{out['best_epoch']}.pt" in best
    m = evaluate_epoch(model, va, str(ann_path), 9, "val", 4, 0, 4, 0.0, 0.9, dev, str(tmp_path / "ev"),
                       metrics="device")
    written = json.load(open(tmp_path / "ev" / "epoch_9_val_metrics.json"))
    assert set(METRIC_KEYS) <= set(written) and written["num_images"] == 6
    assert all(written[k] == m[k] for k in METRIC_KEYS)
