"""Plain-Python restatement of the caption metrics as pycocoevalcap computes them when the reference calls it
(src/eval.py:59-108): raw strings, Bleu(4) with option "closest", Rouge() with beta = 1.2, Cider() with n = 4 and
sigma = 6. Written from the definitions with dict / defaultdict and fp64; it shares no code with icap/metrics.py
and is the yardstick of tests/test_caption_metrics_*.py. Beside the scores it returns the per-image values and the
integer intermediates (BLEU's stats rows, the LCS of every (image, reference) pair).

gts: {image_id: [reference, ...]}, res: {image_id: hypothesis}; only ids in both are scored, in sorted order."""

import math
from collections import defaultdict

import numpy as np

KEYS = ("BLEU-1", "BLEU-2", "BLEU-3", "BLEU-4", "ROUGE-L", "CIDEr")


def common_ids(gts, res):
    ids = sorted(set(gts) & set(res))
    if not ids:
        raise ValueError("No common image IDs found between predictions and references")
    return ids


def precook(s, n=4):
    words = s.split()
    counts = defaultdict(int)
    for k in range(1, n + 1):
        for i in range(len(words) - k + 1):
            counts[tuple(words[i:i + k])] += 1
    return len(words), counts


# ---- BLEU ---------------------------------------------------------------------------------------------------

def bleu_stats(hyp, refs):
    """[testlen, reflen, guess[4], correct[4]] of one image."""
    testlen, counts = precook(hyp)
    reflens, maxcounts = [], {}
    for r in refs:
        rl, rc = precook(r)
        reflens.append(rl)
        for g, c in rc.items():
            maxcounts[g] = max(maxcounts.get(g, 0), c)
    reflen = min((abs(l - testlen), l) for l in reflens)[1]
    guess = [max(0, testlen - k + 1) for k in range(1, 5)]
    correct = [0] * 4
    for g, c in counts.items():
        correct[len(g) - 1] += min(maxcounts.get(g, 0), c)
    return [testlen, reflen] + guess + correct


def _bleu_of(testlen, reflen, guess, correct):
    tiny, small = 1e-15, 1e-9
    out = []
    bleu = 1.0
    for k in range(4):
        bleu *= (float(correct[k]) + tiny) / (float(guess[k]) + small)
        out.append(bleu ** (1.0 / (k + 1)))
    ratio = (testlen + tiny) / (reflen + small)
    if ratio < 1:
        for k in range(4):
            out[k] *= math.exp(1 - 1 / ratio)
    return out


def bleu(gts, res):
    """(corpus BLEU-1..4, per-image [[4]], stats rows [[10]])."""
    ids = common_ids(gts, res)
    rows = [bleu_stats(res[i], gts[i]) for i in ids]
    per = [_bleu_of(r[0], r[1], r[2:6], r[6:10]) for r in rows]
    tot = [sum(r[c] for r in rows) for c in range(10)]
    return _bleu_of(tot[0], tot[1], tot[2:6], tot[6:10]), per, rows


# ---- ROUGE-L ------------------------------------------------------------------------------------------------

def lcs_len(a, b):
    t = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            t[i][j] = t[i - 1][j - 1] + 1 if a[i - 1] == b[j - 1] else max(t[i - 1][j], t[i][j - 1])
    return t[len(a)][len(b)]


def rouge(gts, res):
    """(ROUGE-L, per-image [], lcs per pair [[per reference] per image])."""
    beta = 1.2
    per, pairs = [], []
    for i in common_ids(gts, res):
        token_c = res[i].split(" ")
        prec, rec, ls = [], [], []
        for r in gts[i]:
            token_r = r.split(" ")
            l = lcs_len(token_r, token_c)
            ls.append(l)
            prec.append(l / float(len(token_c)))
            rec.append(l / float(len(token_r)))
        p, q = max(prec), max(rec)
        per.append(((1 + beta ** 2) * p * q) / float(q + beta ** 2 * p) if p != 0 and q != 0 else 0.0)
        pairs.append(ls)
    return float(np.mean(np.array(per))), per, pairs


# ---- CIDEr --------------------------------------------------------------------------------------------------

def cider(gts, res, n=4, sigma=6.0):
    """(CIDEr, per-image [])."""
    ids = common_ids(gts, res)
    crefs = [[precook(r, n)[1] for r in gts[i]] for i in ids]
    ctest = [precook(res[i], n)[1] for i in ids]
    df = defaultdict(float)
    for refs in crefs:
        for g in set(g for ref in refs for g in ref):
            df[g] += 1
    ref_len = np.log(float(len(crefs)))

    def counts2vec(cnts):
        vec = [defaultdict(float) for _ in range(n)]
        length = 0
        norm = [0.0] * n
        for g, tf in cnts.items():
            d = np.log(max(1.0, df[g]))
            k = len(g) - 1
            vec[k][g] = float(tf) * (ref_len - d)
            norm[k] += pow(vec[k][g], 2)
            if k == 1:
                length += tf
        return vec, [np.sqrt(v) for v in norm], length

    def sim(vh, vr, nh, nr, lh, lr):
        delta = float(lh - lr)
        val = np.array([0.0] * n)
        for k in range(n):
            for g in vh[k]:
                val[k] += min(vh[k][g], vr[k][g]) * vr[k][g]
            if nh[k] != 0 and nr[k] != 0:
                val[k] /= nh[k] * nr[k]
            val[k] *= np.e ** (-(delta ** 2) / (2 * sigma ** 2))
        return val

    scores = []
    for test, refs in zip(ctest, crefs):
        vh, nh, lh = counts2vec(test)
        score = np.array([0.0] * n)
        for ref in refs:
            vr, nr, lr = counts2vec(ref)
            score += sim(vh, vr, nh, nr, lh, lr)
        s = np.mean(score)
        s /= len(refs)
        s *= 10.0
        scores.append(float(s))
    return float(np.mean(np.array(scores))), scores


# ---- all three ----------------------------------------------------------------------------------------------

def score(gts, res):
    """{"ids", "metrics" {six keys}, "per_image" {id: {six keys}}, "stats" [[10]], "lcs" [[..]]} over the common ids."""
    ids = common_ids(gts, res)
    b, b_img, stats = bleu(gts, res)
    r, r_img, pairs = rouge(gts, res)
    c, c_img = cider(gts, res)
    metrics = dict(zip(KEYS, b + [r, c]))
    per = {i: dict(zip(KEYS, b_img[j] + [r_img[j], c_img[j]])) for j, i in enumerate(ids)}
    return {"ids": ids, "metrics": metrics, "per_image": per, "stats": stats, "lcs": pairs}
