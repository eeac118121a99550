"""fp64 restatement of caption scoring (include/icap.h icap_caption_score, DESIGN.md "Caption scoring") from
(logits, labels, P), plus the designed kernel cases and bounds of tests/test_score_kernel_gpu.py.

Definitions (the reference's loss, src/models.py:286-325 and HF loss_utils.py:32-71, taken apart per caption): the
rows are [prefix (P) ; caption (Lc)], the full labels [-100] * P ++ labels[b], row i predicts full label i + 1, a
target is a row whose shifted label is not -100. Per caption: nll = sum over targets of logsumexp(x[:V]) - x[y],
n_tokens = number of targets, n_correct = targets whose label is the FIRST maximum of the row's V logits
(torch.argmax's rule, NaN being the maximum), token_logprobs[b, t] = -(lse - x[y]) at the row predicting caption
token t and 0 where labels[b, t] == -100.

Bounds (kernel level): per row |got - ref| <= 1e-5 * max(1, |ref|) (loss_refs.loss_ratio: the fast exponential and
the fp32 lse, see loss_refs); per sequence |got - ref| <= 1e-5 * sum_rows max(1, |ref_r|) + 2^-23 * |ref| (the rows'
errors add; the device adds the fp32 row values exactly in double and rounds once: half an ulp, 2^-24, doubled).
Counts and the zero pattern are exact. Non-finite references (a -inf label logit gives +inf, a NaN in the row gives
NaN) must be reproduced exactly."""

import numpy as np
import torch

SEQ_ULP = 2.0 ** -23
ROW_TOL = 1e-5


def shifted_labels(labels, P):
    """int64 [B, P + Lc]: the label row i predicts (-100 for the last row and the rows predicting a prefix slot)."""
    labels = torch.as_tensor(labels).long()
    B, Lc = labels.shape
    full = torch.cat([torch.full((B, P), -100, dtype=torch.int64), labels], dim=1)
    return torch.cat([full[:, 1:], torch.full((B, 1), -100, dtype=torch.int64)], dim=1)


def row_scores(x, y, V):
    """(nll fp64 [rows] (0 where y < 0), hit bool [rows]) of logits x [rows, >= V] and labels y [rows]."""
    x = torch.as_tensor(x).double()[:, :V]
    y = torch.as_tensor(y).long()
    tgt = y >= 0
    lse = torch.logsumexp(x, dim=1)
    xy = torch.gather(x, 1, y.clamp_min(0)[:, None])[:, 0]
    nll = torch.where(tgt, lse - xy, torch.zeros_like(lse))
    hit = tgt & (first_argmax(x) == y)
    return nll, hit


def first_argmax(x):
    """torch.argmax's rule, spelled out so it does not depend on the library's tie handling: NaN is the maximum, the
    lowest index among equal maxima wins."""
    x = torch.as_tensor(x).double()
    nan = torch.isnan(x)
    key = torch.where(nan, torch.full_like(x, float("inf")), x)
    rank = torch.where(nan, torch.full_like(x, 2.0), torch.where(key == key.max(dim=1, keepdim=True).values,
                                                                  torch.ones_like(x), torch.zeros_like(x)))
    best = rank == rank.max(dim=1, keepdim=True).values
    idx = torch.arange(x.shape[1]).expand_as(x)
    return torch.where(best, idx, torch.full_like(idx, x.shape[1])).min(dim=1).values


def score(logits, labels, P, V=None):
    """logits [B, P + Lc, >= V], labels [B, Lc] -> dict of nll fp64 [B], n_tokens, n_correct int64 [B],
    token_logprobs fp64 [B, Lc], row_nll fp64 [B, S], row_hit bool [B, S], loss (sum nll / sum n_tokens)."""
    logits = torch.as_tensor(logits)
    labels = torch.as_tensor(labels).long()
    B, S = logits.shape[:2]
    Lc = labels.shape[1]
    assert S == P + Lc
    V = logits.shape[2] if V is None else V
    ys = shifted_labels(labels, P)
    nll, hit = row_scores(logits.reshape(B * S, -1), ys.reshape(-1), V)
    nll, hit = nll.view(B, S), hit.view(B, S)
    tlp = torch.zeros((B, Lc), dtype=torch.float64)
    for t in range(Lc):
        if P + t - 1 >= 0:
            tlp[:, t] = torch.where(labels[:, t] != -100, -nll[:, P + t - 1], torch.zeros(B, dtype=torch.float64))
    out = dict(nll=seq_sum(nll), n_tokens=(ys >= 0).sum(1), n_correct=hit.sum(1), token_logprobs=tlp, row_nll=nll,
               row_hit=hit)
    nt = int(out["n_tokens"].sum())
    out["loss"] = float(out["nll"].sum()) / nt if nt else float("nan")
    return out


def seq_sum(nll_rows):
    """Row-order double sum per sequence of [B, S]."""
    out = torch.zeros(nll_rows.shape[0], dtype=torch.float64)
    for s in range(nll_rows.shape[1]):
        out = out + nll_rows[:, s]
    return out


def same_nonfinite(got, ref):
    """Where ref is not finite, got holds the same value (NaN for NaN, the same infinity)."""
    got, ref = torch.as_tensor(got).double().cpu().reshape(-1), torch.as_tensor(ref).double().reshape(-1)
    bad = ~torch.isfinite(ref)
    g, r = got[bad], ref[bad]
    return bool(torch.isfinite(got[~bad]).all() and ((g == r) | (torch.isnan(g) & torch.isnan(r))).all())


def finite(got, ref):
    got, ref = torch.as_tensor(got).double().cpu().reshape(-1), torch.as_tensor(ref).double().reshape(-1)
    ok = torch.isfinite(ref)
    return got[ok], ref[ok]


def seq_ratio(got, ref_rows, ranges):
    """Worst |got[b] - ref[b]| / (1e-5 * sum_r max(1, |ref_r|) + 2^-23 |ref[b]|) over the sequences whose reference
    is finite; ref_rows fp64 [rows] (0 on ignored rows), ranges [(r0, r1)]."""
    worst = 0.0
    got = torch.as_tensor(got).double().cpu()
    for b, (r0, r1) in enumerate(ranges):
        rows = ref_rows[r0:r1]
        ref = float(seq_sum(rows[None])[0]) if r1 > r0 else 0.0
        if not np.isfinite(ref):
            continue
        live = rows[rows != 0]
        tol = ROW_TOL * float(live.abs().clamp_min(1.0).sum()) + SEQ_ULP * abs(ref)
        d = abs(float(got[b]) - ref)
        worst = max(worst, d / tol if tol > 0 else (0.0 if d == 0 else float("inf")))
    return worst


# ---------------------------------------------------------------------------------------------- designed kernel case

SEQ_TARGETS = (0, 1, 3, 9, 2)   # targets per sequence
NEG_INF_LABEL_ROW = 3           # target index (over all 15; in sequence 2) whose label logit is -inf: nll = +inf
NAN_ROW = 11                    # target index (in sequence 3) whose row holds a NaN


def designed_targets(V, ld, dtype, seed=7, nonfinite=True):
    """The 15 target rows as (logits [15, ld] in `dtype`, labels int32 [15]). Values N(0, 2^2) rounded to dtype;
    padding columns V..ld alternate +1e30 and NaN (never read). Even targets: the label is the maximum (raised above
    the row); target 2: an exact tie with the label BEFORE the other maximum (label wins), target 4: the label AFTER
    the other maximum (label loses); targets 6, 7: -inf logits off the label; target 3: x[y] = -inf; target 11: a
    NaN off the label (nll NaN; the NaN is the argmax, so no hit); nonfinite=False leaves those two rows plain (every
    nll finite, for the running totals). V = 13 keeps every special index inside the row."""
    g = torch.Generator().manual_seed(seed + V)
    n = sum(SEQ_TARGETS)
    x = (2.0 * torch.randn((n, ld), generator=g)).to(dtype).float()
    y = torch.randint(0, V, (n,), generator=g, dtype=torch.int64)
    lo, hi = 2, V - 3
    y[0], y[1], y[2], y[4] = V - 1, 0, lo, hi  # the V % 8 tail column, column 0, the two tie rows
    top = 16.0  # exact in bf16, above every N(0, 4) draw
    for r in range(n):
        if r % 2 == 0:
            x[r, y[r]] = top
    x[2, hi] = top                     # tie, label first: a hit
    x[4, lo] = top                     # tie, label second: no hit
    for r in (6, 7):
        cols = [c for c in range(V) if c != int(y[r])][:: max(1, V // 5)]
        x[r, cols] = float("-inf")
    if nonfinite:
        x[NEG_INF_LABEL_ROW, y[NEG_INF_LABEL_ROW]] = float("-inf")
        x[NAN_ROW, (int(y[NAN_ROW]) + 1) % V] = float("nan")
    if ld > V:
        x[:, V:] = 1e30
        x[:, V + 1:: 2] = float("nan")
    return x.to(dtype), y.to(torch.int32)


def padded_layout(xt, yt, S=12, dead=float("nan")):
    """The padded-grid form: 5 sequences of S rows, each sequence's targets interleaved with -100 rows (every other
    row from row 1 on, the rest after them). Returns logits [5 S, ld], labels int32 [5 S], ranges int32 [6].
    Ignored rows hold random finite logits."""
    B = len(SEQ_TARGETS)
    ld = xt.shape[1]
    g = torch.Generator().manual_seed(3)
    x = torch.randn((B * S, ld), generator=g).to(xt.dtype)
    y = torch.full((B * S,), -100, dtype=torch.int32)
    k = 0
    for b, n in enumerate(SEQ_TARGETS):
        pos = [1 + 2 * i for i in range(n) if 1 + 2 * i < S]
        pos += [p for p in range(S) if p not in pos][: n - len(pos)]
        for p in sorted(pos):
            x[b * S + p] = xt[k]
            y[b * S + p] = yt[k]
            k += 1
    ranges = torch.arange(B + 1, dtype=torch.int32) * S
    return x, y, ranges


def compact_layout(xt, yt, extra=4):
    """The compact form: the 15 target rows back to back, then `extra` rows past rows_dev filled with NaN (labels
    0: they would score if read). Returns logits, labels, ranges int32 [6], live (= 15)."""
    n = xt.shape[0]
    x = torch.cat([xt, torch.full((extra, xt.shape[1]), float("nan")).to(xt.dtype)])
    y = torch.cat([yt, torch.zeros(extra, dtype=torch.int32)])
    ranges = torch.tensor(np.concatenate([[0], np.cumsum(SEQ_TARGETS)]), dtype=torch.int32)
    return x, y, ranges, n
