"""BLEU-1..4, ROUGE-L and CIDEr without pycocoevalcap: counted on the device, finished on the host.

The definitions are pycocoevalcap's as the reference calls it (src/eval.py:59-108): raw strings (no PTB tokeniser),
Bleu(4) with the "closest" reference length, Rouge() with beta = 1.2 and Cider() with n = 4, sigma = 6. BLEU and
CIDEr tokenise with str.split(), ROUGE-L with str.split(" "); both token lists are packed, over one dictionary.

The host's share: tokenise, map words to int32 ids, pack, and turn the device's exact integers (BLEU's counts, the
LCS lengths) into floats in the library's arithmetic order. The device's share (csrc/caption_metrics.hip): n-gram
identity, document frequencies, clipped counts, LCS, and CIDEr per image in fp64. There is no CPU path.
"""

from __future__ import annotations

import math
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from .evaluate import METRIC_KEYS

MAX_WORDS = L.METRIC_MAX_WORDS  # ICAP_METRIC_MAX_WORDS: a longer caption is refused, never truncated
ROUGE_BETA = 1.2


# ---- host packing (pure, no GPU) --------------------------------------------------------------------------------

def tokenize(s: str) -> Tuple[List[str], List[str]]:
    """(BLEU / CIDEr tokens, ROUGE-L tokens): split on any whitespace run, and on single spaces ("" is one empty
    token, "a  b " is ["a", "", "b", ""])."""
    return s.split(), s.split(" ")


class PackedCaptions:
    """Rows of captions as int32 word ids: words_a / ptr_a (str.split()) and words_b / ptr_b (str.split(" "))."""

    __slots__ = ("words_a", "ptr_a", "words_b", "ptr_b")

    def __init__(self, words_a, ptr_a, words_b, ptr_b):
        self.words_a, self.ptr_a, self.words_b, self.ptr_b = words_a, ptr_a, words_b, ptr_b

    def __len__(self) -> int:
        return len(self.ptr_a) - 1


def pack_captions(captions: Sequence[str], image_ids: Sequence, vocab: Dict[str, int]) -> PackedCaptions:
    """Tokenise `captions` both ways and map the words through `vocab`, which grows by the words it has not seen (the
    empty token and tokens holding newlines are ordinary entries). image_ids[i] names caption i in the error a
    caption of more than MAX_WORDS tokens raises."""
    wa: List[int] = []
    wb: List[int] = []
    pa, pb = [0], [0]
    for s, iid in zip(captions, image_ids):
        ta, tb = tokenize(s)
        if len(ta) > MAX_WORDS or len(tb) > MAX_WORDS:
            raise ValueError(f"caption of image {iid} has {max(len(ta), len(tb))} tokens; the device metrics take at "
                             f"most {MAX_WORDS} (ICAP_METRIC_MAX_WORDS) and do not truncate")
        for toks, out in ((ta, wa), (tb, wb)):
            for t in toks:
                i = vocab.get(t)
                if i is None:
                    i = vocab[t] = len(vocab)
                out.append(i)
        pa.append(len(wa))
        pb.append(len(wb))
    i32 = np.int32
    return PackedCaptions(np.asarray(wa, dtype=i32), np.asarray(pa, dtype=i32), np.asarray(wb, dtype=i32),
                          np.asarray(pb, dtype=i32))


def select_common(predictions, reference_ids) -> Tuple[list, Dict]:
    """(sorted ids of the images present in both, {id: hypothesis}). predictions: [{"image_id", "caption"}] (a later
    entry of an image replaces an earlier one) or {id: [caption]}."""
    if isinstance(predictions, dict):
        res = {k: (v[0] if isinstance(v, (list, tuple)) else v) for k, v in predictions.items()}
    else:
        res = {p["image_id"]: p["caption"] for p in predictions}
    common = sorted(set(res) & set(reference_ids))
    if not common:
        raise ValueError("No common image IDs found between predictions and references")
    return common, res


def ngram_positions(ptr: np.ndarray, rows=None) -> Tuple[int, int, int]:
    """Number of 2-, 3-, 4-gram start positions in the packed rows (all, or the listed ones)."""
    n = np.diff(ptr.astype(np.int64))
    if rows is not None:
        n = n[rows]
    return tuple(int(np.maximum(n - k + 1, 0).sum()) for k in (2, 3, 4))


# ---- host finishing (pure, no GPU) ------------------------------------------------------------------------------

def _bleu_row(testlen, reflen, guess, correct) -> List[float]:
    tiny, small = 1e-15, 1e-9
    out = []
    b = 1.0
    for k in range(4):
        b *= (float(correct[k]) + tiny) / (float(guess[k]) + small)
        out.append(b ** (1.0 / (k + 1)))
    ratio = (testlen + tiny) / (reflen + small)
    if ratio < 1:
        f = math.exp(1 - 1 / ratio)
        out = [v * f for v in out]
    return out


def bleu_from_stats(stats, per_image: bool = True) -> Tuple[List[float], np.ndarray]:
    """stats int [I, 10] = testlen, reflen, guess[4], correct[4] per image -> (corpus BLEU-1..4, per-image [I, 4]):
    Bleu(4).compute_score with option "closest", on the summed counts and on each image's own (per_image=False
    skips those: an empty [0, 4])."""
    st = np.asarray(stats, dtype=np.int64).reshape(-1, 10)
    rows = st.tolist() if per_image else []
    per = np.array([_bleu_row(r[0], r[1], r[2:6], r[6:10]) for r in rows], dtype=np.float64).reshape(-1, 4)
    tot = st.sum(axis=0).tolist()
    return _bleu_row(tot[0], tot[1], tot[2:6], tot[6:10]), per


def rouge_from_lcs(lcs, hyp_len, ref_len, ref_ptr) -> Tuple[float, np.ndarray]:
    """lcs / ref_len per (image, reference) pair, hyp_len per image (split(" ") token counts), ref_ptr [I + 1] the
    pairs of each image (at least one each) -> (ROUGE-L, per-image [I]): Rouge().compute_score, beta = 1.2. The
    library's operations in its order, element by element in numpy fp64."""
    beta = ROUGE_BETA
    lcs = np.asarray(lcs, dtype=np.float64)
    ptr = np.asarray(ref_ptr, dtype=np.int64)
    hyp_len = np.asarray(hyp_len, dtype=np.float64)
    prec = lcs / np.repeat(hyp_len, np.diff(ptr))
    rec = lcs / np.asarray(ref_len, dtype=np.float64)
    p, r = np.maximum.reduceat(prec, ptr[:-1]), np.maximum.reduceat(rec, ptr[:-1])
    both = (p != 0) & (r != 0)
    den = np.where(both, r + beta ** 2 * p, 1.0)
    per = np.where(both, ((1 + beta ** 2) * p * r) / den, 0.0)
    return float(np.mean(per)), per


# ---- the scorer -------------------------------------------------------------------------------------------------

class MetricsBatch:
    """One score() call's device inputs and outputs (DeviceCaptionMetrics.pack): what ops.caption_metrics takes."""

    def __init__(self, ids, arrays, n_vocab, n_ref_words, n_hyp_words, positions, hyp_len_b, ref_len_b, pair_ptr,
                 device):
        self.ids, self.arrays = ids, arrays
        self.n_images = len(ids)
        self.n_vocab, self.n_ref_words, self.n_hyp_words = n_vocab, n_ref_words, n_hyp_words
        self.positions = positions
        self.hyp_len_b, self.ref_len_b, self.pair_ptr = hyp_len_b, ref_len_b, pair_ptr
        n_pairs = int(pair_ptr[-1])
        # one buffer, so one copy reads everything back: cider fp64 [I] | stats int32 [I, 10] | lcs [pairs] | flag
        self.out = torch.zeros(8 * self.n_images + 4 * (10 * self.n_images + n_pairs + 1), dtype=torch.uint8,
                               device=device)
        I = self.n_images
        self.cider = self.out[:8 * I].view(torch.float64)
        ints = self.out[8 * I:].view(torch.int32)
        self.stats, self.lcs, self.flag = ints[:10 * I].view(I, 10), ints[10 * I:10 * I + n_pairs], ints[-1:]

    def kwargs(self, capacities, workspace, stages: int = 0) -> dict:
        return dict(n_images=self.n_images, n_vocab=self.n_vocab, n_ref_words=self.n_ref_words,
                    n_hyp_words=self.n_hyp_words, positions=self.positions, capacities=capacities,
                    workspace=workspace, stats=self.stats, lcs=self.lcs, cider=self.cider, flag=self.flag,
                    stages=stages)

    def read(self):
        """(stats [I, 10], lcs [pairs], cider [I]) on the host: the one synchronising copy."""
        host = self.out.cpu().numpy()
        I = self.n_images
        cider = host[:8 * I].view(np.float64).copy()
        ints = host[8 * I:].view(np.int32)
        if ints[-1] != 0:
            raise L.IcapError("caption metrics: an n-gram table filled up (positions understated)")
        return ints[:10 * I].reshape(I, 10).copy(), ints[10 * I:-1].copy(), cider


class DeviceCaptionMetrics:
    """The reference captions of one annotations file, tokenised, packed and resident on the device.

    references: {image_id: [caption, ...]} or the path of a COCO annotations JSON. score(predictions) returns
    {"BLEU-1", ..., "BLEU-4", "ROUGE-L", "CIDEr"} over the images present in both, as pycocoevalcap computes them;
    per_image=True adds "per_image": {image_id: {the six keys}}."""

    def __init__(self, references, device=None):
        if isinstance(references, (str, bytes)) or hasattr(references, "__fspath__"):
            from .evaluate import load_coco_references

            references = load_coco_references(references)
        self.device = torch.device(device) if device is not None else torch.device("cuda")
        if self.device.type == "cuda" and not torch.cuda.is_available():
            raise L.IcapError("DeviceCaptionMetrics needs a GPU: the caption metrics have no CPU path")
        L.require_device(self.device)
        self.image_ids = list(references)
        self.image_index = {iid: i for i, iid in enumerate(self.image_ids)}
        caps, owners, ptr = [], [], [0]
        for iid in self.image_ids:
            refs = references[iid]
            if len(refs) < 1:
                raise ValueError(f"image {iid} has no reference caption")
            caps += list(refs)
            owners += [iid] * len(refs)
            ptr.append(len(caps))
        self.vocab: Dict[str, int] = {}
        self.refs = pack_captions(caps, owners, self.vocab)
        self.img_ref_ptr = np.asarray(ptr, dtype=np.int32)
        self.ref_len_a = np.diff(self.refs.ptr_a)
        self.ref_len_b = np.diff(self.refs.ptr_b)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)  # noqa: E731
        pad = lambda a: a if len(a) else np.zeros(1, dtype=np.int32)  # noqa: E731  (a tensor needs an address)
        self._dev = {"img_ref_ptr": up(self.img_ref_ptr), "ref_ptr_a": up(self.refs.ptr_a),
                     "ref_words_a": up(pad(self.refs.words_a)), "ref_ptr_b": up(self.refs.ptr_b),
                     "ref_words_b": up(pad(self.refs.words_b))}
        self._workspace = None

    def pack(self, predictions) -> MetricsBatch:
        """Select the common images, pack their hypotheses (extending the dictionary) and upload them in one copy."""
        ids, res = select_common(predictions, self.image_index)
        hyp = pack_captions([res[i] for i in ids], ids, self.vocab)
        sel = np.asarray([self.image_index[i] for i in ids], dtype=np.int32)
        m = (self.img_ref_ptr[1:] - self.img_ref_ptr[:-1])[sel]
        pair_ptr = np.concatenate([[0], np.cumsum(m)]).astype(np.int32)
        rows = np.concatenate([np.arange(self.img_ref_ptr[s], self.img_ref_ptr[s + 1]) for s in sel])
        pos_r = ngram_positions(self.refs.ptr_a, rows)
        pos_h = ngram_positions(hyp.ptr_a)
        parts = {"sel": sel, "hyp_ptr_a": hyp.ptr_a, "hyp_words_a": hyp.words_a, "hyp_ptr_b": hyp.ptr_b,
                 "hyp_words_b": hyp.words_b, "pair_ptr": pair_ptr}
        offs, total = {}, 0
        for k, v in parts.items():
            offs[k] = total
            total += max(len(v), 1)
        host = np.zeros(total, dtype=np.int32)
        for k, v in parts.items():
            host[offs[k]:offs[k] + len(v)] = v
        dev = torch.from_numpy(host).to(self.device)
        arrays = dict(self._dev)
        for k, v in parts.items():
            arrays[k] = dev[offs[k]:offs[k] + max(len(v), 1)]
        return MetricsBatch(ids, arrays, len(self.vocab), len(self.refs.words_a), len(hyp.words_a),
                            tuple(a + b for a, b in zip(pos_r, pos_h)), np.diff(hyp.ptr_b), self.ref_len_b[rows],
                            pair_ptr, self.device)

    def workspace(self, batch: MetricsBatch, capacities) -> torch.Tensor:
        """The pass's scratch memory, kept between calls and grown when a call needs more."""
        from . import ops

        need = ops.caption_metrics_workspace(batch.n_vocab, batch.n_ref_words, batch.n_hyp_words, capacities)
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._workspace

    def device_pass(self, predictions, capacities=None):
        """(image ids, stats int32 [I, 10], lcs int32 [pairs], cider float64 [I], the batch) of one pass."""
        from . import ops

        batch = self.pack(predictions)
        caps = capacities if capacities is not None else ops.caption_metrics_capacities(batch.positions)
        with torch.cuda.device(self.device):
            ops.caption_metrics(batch.arrays, **batch.kwargs(caps, self.workspace(batch, caps)))
            stats, lcs, cider = batch.read()
        return batch.ids, stats, lcs, cider, batch

    def score(self, predictions, per_image: bool = False) -> dict:
        ids, stats, lcs, cider, batch = self.device_pass(predictions)
        bleu, bleu_img = bleu_from_stats(stats, per_image=per_image)
        rouge, rouge_img = rouge_from_lcs(lcs, batch.hyp_len_b, batch.ref_len_b, batch.pair_ptr)
        out = {k: float(v) for k, v in zip(METRIC_KEYS[:4], bleu)}
        out["ROUGE-L"] = rouge
        out["CIDEr"] = float(np.mean(cider))
        if per_image:
            out["per_image"] = {
                iid: {**{k: float(bleu_img[i, j]) for j, k in enumerate(METRIC_KEYS[:4])},
                      "ROUGE-L": float(rouge_img[i]), "CIDEr": float(cider[i])}
                for i, iid in enumerate(ids)}
        return out
