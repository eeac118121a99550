"""Caption metrics without a GPU: the restatement against the worked example, the host packing and selection of
icap/metrics.py, its host finishing (bleu_from_stats, rouge_from_lcs) against the restatement's floats on the
restatement's integers, the library's argument checks (before any HIP call), and the opt-in plumbing."""

import ctypes as C
import random

import numpy as np
import pytest

import caption_metric_refs as R
from icap import _lib, metrics as M
from icap.evaluate import compute_caption_metrics

ANCHOR_REFS = {1: ["a cat sits on the mat", "the cat is on a mat "],
               2: ["two dogs run in a park", "dogs running in the park", "two dogs in a park"],
               3: ["a man rides a red bike"]}
ANCHOR_RES = {1: "a cat on the mat", 2: "two dogs run in the the park", 3: "a man rides a bike  fast"}
ANCHOR = {"BLEU-1": 0.8888888887901234, "BLEU-2": 0.8073734276651375, "BLEU-3": 0.6476085202809216,
          "BLEU-4": 0.4956570491080505, "ROUGE-L": 0.8181768180943166, "CIDEr": 4.097299678904853}


def random_corpus(seed, n_images=64, vocab=12, max_refs=7, max_len=128):
    """{id: [references]}, {id: hypothesis}: 1..max_refs references, lengths 0..max_len, single and double spaces and
    trailing whitespace so the two tokenisations differ."""
    rng = random.Random(seed)
    words = [f"w{i}" for i in range(vocab)]

    def caption():
        n = rng.choice([0, 1, 2, 3, max_len]) if rng.random() < 0.15 else rng.randint(0, max_len)
        s = " ".join(rng.choice(words) for _ in range(n))
        extra = 0  # empty split(" ") tokens added: never more than max_len tokens under either tokenisation
        if n >= 2 and n + extra < max_len and rng.random() < 0.3:
            s = s.replace(" ", "  ", 1)
            extra += 1
        if n >= 1 and n + extra < max_len and rng.random() < 0.3:
            s += rng.choice([" ", "\n"])
        return s

    gts = {100 + 3 * i: [caption() for _ in range(rng.randint(1, max_refs))] for i in range(n_images)}
    res = {i: caption() for i in gts}
    return gts, res


def test_restatement_reproduces_the_anchor():
    out = R.score(ANCHOR_REFS, ANCHOR_RES)
    for k, want in ANCHOR.items():
        assert abs(out["metrics"][k] - want) <= 1e-12, (k, out["metrics"][k], want)
    # BLEU-1 by hand: 5/5, 6/7 (the doubled "the" clipped to 1), 5/6; lengths 18 against 18
    assert [r[6] for r in out["stats"]] == [5, 6, 5] and [r[2] for r in out["stats"]] == [5, 7, 6]
    assert sum(r[0] for r in out["stats"]) == sum(r[1] for r in out["stats"]) == 18


def test_tokenisations():
    assert M.tokenize("a  b ") == (["a", "b"], ["a", "", "b", ""])
    assert M.tokenize("") == ([], [""])
    assert M.tokenize("x\n") == (["x"], ["x\n"])


def test_packing_one_dictionary_and_row_pointers():
    vocab = {}
    refs = M.pack_captions(["a  b ", "", "x\n"], [7, 7, 8], vocab)
    assert refs.ptr_a.tolist() == [0, 2, 2, 3] and refs.ptr_b.tolist() == [0, 4, 5, 6]
    assert refs.words_a.dtype == np.int32 and refs.ptr_a.dtype == np.int32
    inv = {v: k for k, v in vocab.items()}
    assert [inv[i] for i in refs.words_a] == ["a", "b", "x"]
    assert [inv[i] for i in refs.words_b] == ["a", "", "b", "", "", "x\n"]  # "" and "x\n" are ordinary words
    n = len(vocab)
    hyp = M.pack_captions(["b a q"], [7], vocab)  # the hypotheses extend the same dictionary
    assert len(vocab) == n + 1 and len(hyp) == 1
    assert [inv.get(i, "q") for i in hyp.words_a] == ["b", "a", "q"]
    assert hyp.words_a[0] == vocab["b"] == refs.words_a[1]
    assert M.ngram_positions(refs.ptr_a) == (1, 0, 0)
    assert M.ngram_positions(np.array([0, 5, 7, 7]), rows=[0, 1]) == (5, 3, 2)


def test_word_cap():
    ok = " ".join(["w"] * M.MAX_WORDS)
    assert M.MAX_WORDS == 128 == _lib.METRIC_MAX_WORDS
    assert len(M.pack_captions([ok], [5], {}).words_a) == 128
    with pytest.raises(ValueError, match="image 4711"):
        M.pack_captions([ok, ok + " w"], [5, 4711], {})
    with pytest.raises(ValueError, match="image 12"):  # 129 tokens under split(" ") only
        M.pack_captions(["a " * 128], [12], {})


def test_common_selection():
    preds = [{"image_id": 2, "caption": "first"}, {"image_id": 9, "caption": "x"}, {"image_id": 2, "caption": "last"},
             {"image_id": 1, "caption": "one"}]
    ids, res = M.select_common(preds, {1: 0, 2: 1, 3: 2})
    assert ids == [1, 2] and res[2] == "last" and res[1] == "one"
    ids, res = M.select_common({3: ["three"], 5: ["five"]}, {1: 0, 2: 1, 3: 2})
    assert ids == [3] and res[3] == "three"
    with pytest.raises(ValueError, match="No common image IDs found between predictions and references"):
        M.select_common([{"image_id": 9, "caption": "x"}], {1: 0})


@pytest.mark.parametrize("case", ["anchor", "small_vocab", "large_vocab"])
def test_host_finishing_matches_the_restatement(case):
    gts, res = {"anchor": lambda: (ANCHOR_REFS, ANCHOR_RES), "small_vocab": lambda: random_corpus(1, 24, 12, 7, 40),
                "large_vocab": lambda: random_corpus(2, 24, 5000, 7, 40)}[case]()
    want = R.score(gts, res)
    ids = want["ids"]
    bleus, per = M.bleu_from_stats(np.array(want["stats"], dtype=np.int32))
    rel = lambda a, b: abs(a - b) <= 1e-12 * abs(b)  # noqa: E731
    for k in range(4):
        assert rel(bleus[k], want["metrics"][R.KEYS[k]])
        for j, i in enumerate(ids):
            assert rel(per[j, k], want["per_image"][i][R.KEYS[k]])
    lcs = np.array([v for ls in want["lcs"] for v in ls], dtype=np.int32)
    ptr = np.concatenate([[0], np.cumsum([len(ls) for ls in want["lcs"]])])
    hyp_len = [len(res[i].split(" ")) for i in ids]
    ref_len = [len(r.split(" ")) for i in ids for r in gts[i]]
    rouge, rper = M.rouge_from_lcs(lcs, hyp_len, ref_len, ptr)
    assert rel(rouge, want["metrics"]["ROUGE-L"])
    for j, i in enumerate(ids):
        assert rel(rper[j], want["per_image"][i]["ROUGE-L"])


def _args(**kw):
    a = _lib.CaptionMetricsArgs()
    for f, _ in a._fields_:
        if f not in ("n_images", "stages", "n_vocab", "n_ref_words", "n_hyp_words", "positions", "capacity",
                     "workspace_bytes"):
            setattr(a, f, 1 << 20)  # never dereferenced: the checks are host-only
    a.n_images, a.n_vocab, a.n_ref_words, a.n_hyp_words = 2, 10, 40, 12
    for k in range(3):
        a.positions[k], a.capacity[k] = 30, 64
    a.workspace_bytes = 1 << 30
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_library_argument_checks_without_gpu():
    a = _args()
    a.capacity[1] = 16  # a power of two, not greater than 30 positions
    with pytest.raises(_lib.IcapError, match="greater than the number of n-gram positions"):
        _lib.call("icap_caption_metrics", C.addressof(a), None)
    a = _args()
    a.capacity[2], a.positions[2] = 32, 32  # equal is refused too
    with pytest.raises(_lib.IcapError, match="greater than"):
        _lib.call("icap_caption_metrics", C.addressof(a), None)
    a = _args()
    a.capacity[0] = 48
    with pytest.raises(_lib.IcapError, match="power of two"):
        _lib.call("icap_caption_metrics", C.addressof(a), None)
    for field in ("sel", "ref_words_b", "hyp_ptr_a", "workspace", "cider", "flag"):
        with pytest.raises(_lib.IcapError, match="null pointer"):
            a = _args(**{field: None})
            _lib.call("icap_caption_metrics", C.addressof(a), None)
    with pytest.raises(_lib.IcapError, match="null args"):
        _lib.call("icap_caption_metrics", None, None)
    with pytest.raises(_lib.IcapError, match="workspace too small"):
        a = _args(workspace_bytes=64)
        _lib.call("icap_caption_metrics", C.addressof(a), None)
    with pytest.raises(_lib.IcapError, match="n_images"):
        a = _args(n_images=0)
        _lib.call("icap_caption_metrics", C.addressof(a), None)


def test_workspace_size_and_capacities():
    from icap import ops

    assert ops.caption_metrics_capacities((0, 1, 5)) == (2, 2, 16)
    assert ops.caption_metrics_capacities((8, 9, 300000)) == (16, 32, 1 << 20)
    small = ops.caption_metrics_workspace(10, 40, 12, (64, 64, 64))
    assert small >= 3 * 64 * 12 + 10 * 4 + 52 * 12
    assert ops.caption_metrics_workspace(10, 40, 12, (128, 64, 64)) > small
    assert ops.caption_metrics_workspace(10, 40, 12, (0, 64, 64)) == 0


def test_struct_layout_matches_header():
    import os
    import subprocess
    import tempfile

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    struct, cname = _lib.CaptionMetricsArgs, "icap_caption_metrics_args"
    fields = [f for f, _ in struct._fields_]
    prog = ["#include <stdio.h>", "#include <stddef.h>", '#include "icap.h"', "int main(void){",
            f'printf("%zu\\n", sizeof({cname}));']
    prog += [f'printf("%zu\\n", offsetof({cname}, {f}));' for f in fields]
    prog += ["return 0;}"]
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write("\n".join(prog))
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), c, "-o", exe])
        vals = [int(x) for x in subprocess.check_output([exe]).split()]
    assert vals[0] == C.sizeof(struct)
    for f, off in zip(fields, vals[1:]):
        assert getattr(struct, f).offset == off, f


def test_backend_plumbing(tmp_path):
    import json

    import icap
    from icap.train import _check_caption_metrics

    preds = [{"image_id": 1, "caption": "a cat"}]
    ann = tmp_path / "ann.json"
    ann.write_text(json.dumps({"annotations": [{"image_id": 1, "caption": "a cat sits"}]}))
    with pytest.raises(ValueError, match="nope"):
        compute_caption_metrics(preds, str(ann), backend="nope")
    assert compute_caption_metrics(preds, str(ann)) == {}  # the default: pycocoevalcap, which is not installed
    assert icap.DeviceCaptionMetrics is M.DeviceCaptionMetrics
    with pytest.raises(ValueError, match="caption_metrics must be"):
        _check_caption_metrics("nope")
    with pytest.raises(ValueError, match="caption_metrics must be"):
        icap.train(None, None, batch_size=1, num_epochs=1, caption_metrics="cpu")
    import torch

    if not torch.cuda.is_available():  # no CPU path and no fallback: a missing device raises
        with pytest.raises(_lib.IcapError):
            M.DeviceCaptionMetrics({1: ["a cat sits"]})
