"""CPU-only checks of the caption-scoring restatement (tests/score_refs.py) and of the argument rules around it:
the restatement reproduces the reference's golden losses from the reference's golden logits, holds its tie / ignored /
infinity rules, tells deliberately wrong restatements apart, and train()'s new arguments validate before any work
while its defaults return what they returned before."""

import math
import os

import numpy as np
import pytest
import torch

import score_refs as R

GOLD = os.path.join(os.path.dirname(__file__), "golden")
P = 5


def _gold(name):
    return dict(np.load(os.path.join(GOLD, name + ".npz")))


@pytest.mark.parametrize("name", ["tiny", "rat_tiny", "tiny_mlp"])
def test_restatement_gives_the_golden_loss(name):
    """sum nll / sum n_tokens over the reference's logits is the reference's loss (stored from an fp32 value)."""
    g = _gold(name)
    s = R.score(g["logits"], g["labels"], P)
    d = abs(s["loss"] - float(g["loss"][0]))
    print(name, "loss", s["loss"], "golden", float(g["loss"][0]), "diff", d, "nll", s["nll"].tolist())
    assert d < 1e-6
    assert s["n_tokens"].tolist() == (torch.from_numpy(g["labels"]) != -100).sum(1).tolist()
    # token_logprobs: minus the per-caption nll when summed, zero exactly where the label is ignored
    assert torch.allclose(-s["token_logprobs"].sum(1), s["nll"], rtol=0, atol=1e-9)
    assert torch.equal(s["token_logprobs"] == 0, torch.from_numpy(g["labels"]) == -100)


def test_tiny_per_caption_values():
    g = _gold("tiny")
    s = R.score(g["logits"], g["labels"], P)
    assert s["n_tokens"].tolist() == [8, 8, 8]
    assert np.allclose(s["nll"].numpy(), [50.58, 50.34, 49.96], atol=0.01), s["nll"]
    # the golden's own argmax of every row agrees with the restatement's first-maximum rule
    assert torch.equal(R.first_argmax(torch.from_numpy(g["logits"]).reshape(-1, 512)),
                       torch.from_numpy(g["argmax"]).reshape(-1))


def _one(x, y, V=None):
    """A single caption of len(y) tokens with P = 1 from rows x [1 + len(y), ld]."""
    x = torch.tensor(x, dtype=torch.float64)[None]
    return R.score(x, torch.tensor([y]), 1, V=V)


def test_ties_go_to_the_lower_index():
    # row 0 predicts token 0, row 1 predicts token 1, the last row predicts nothing
    rows = [[1.0, 3.0, 3.0, 0.0], [2.0, 0.0, 2.0, 2.0], [9.0, 0.0, 0.0, 0.0]]
    assert _one(rows, [1, 0])["n_correct"].tolist() == [2]      # both labels are the first maximum
    assert _one(rows, [2, 2])["n_correct"].tolist() == [0]      # both labels tie but come second
    assert _one(rows, [2, 3])["n_correct"].tolist() == [0]
    s = _one(rows, [1, 0])
    ref = (math.log(math.e + 2 * math.e ** 3 + 1) - 3.0) + (math.log(3 * math.e ** 2 + 1) - 2.0)
    assert abs(float(s["nll"][0]) - ref) < 1e-12


def test_nan_is_the_maximum_and_the_first_nan_wins():
    nan = float("nan")
    rows = [[1.0, nan, 5.0, nan], [0.0, 0.0, 0.0, 0.0]]
    assert _one(rows, [1])["n_correct"].tolist() == [1]
    assert _one(rows, [3])["n_correct"].tolist() == [0]
    assert _one(rows, [2])["n_correct"].tolist() == [0]
    assert math.isnan(float(_one(rows, [2])["nll"][0]))
    x = torch.tensor([[1.0, nan, 5.0, nan], [nan, nan, 0.0, 1.0], [float("inf"), 2.0, nan, 0.0]])
    assert torch.equal(R.first_argmax(x), torch.argmax(x, dim=1))


def test_all_ignored_caption_scores_zero():
    x = torch.randn((2, 4, 8), generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    labels = torch.tensor([[-100, -100, -100], [3, -100, 1]])
    s = R.score(x, labels, 1)
    assert s["nll"][0] == 0 and s["n_tokens"].tolist() == [0, 2] and s["n_correct"][0] == 0
    assert torch.equal(s["token_logprobs"][0], torch.zeros(3, dtype=torch.float64))
    assert torch.equal(s["token_logprobs"][1] == 0, torch.tensor([False, True, False]))
    # the batch ratio ignores the empty caption; with nothing but ignored labels there is no loss
    assert abs(s["loss"] - float(s["nll"][1]) / 2) < 1e-15
    assert math.isnan(R.score(x[:1], labels[:1], 1)["loss"])


def test_infinite_logits():
    inf = float("inf")
    rows = [[0.0, -inf, 1.0, -inf], [0.0, 0.0, 0.0, 0.0]]
    s = _one(rows, [2])                      # -inf off the label: they drop out of the sum
    assert abs(float(s["nll"][0]) - (math.log(1 + math.e) - 1.0)) < 1e-12 and s["n_correct"].tolist() == [1]
    s = _one(rows, [1])                      # x[y] = -inf: nll = +inf, counted, not correct
    assert float(s["nll"][0]) == inf and s["n_tokens"].tolist() == [1] and s["n_correct"].tolist() == [0]
    s = _one([[0.0, inf, 1.0, 2.0], [0.0] * 4], [2])   # a +inf logit off the label: lse = +inf
    assert float(s["nll"][0]) == inf and s["n_correct"].tolist() == [0]
    s = _one([[0.0, inf, 1.0, 2.0], [0.0] * 4], [1])   # +inf at the label: inf - inf
    assert math.isnan(float(s["nll"][0])) and s["n_correct"].tolist() == [1]


# ------------------------------------------------------------------------- deliberately wrong restatements must fail

def _tiny_rows():
    g = _gold("tiny")
    return g, torch.from_numpy(g["logits"]), torch.from_numpy(g["labels"])


def test_unshifted_labels_miss_the_golden_loss():
    g, x, labels = _tiny_rows()
    B, S, V = x.shape
    full = torch.cat([torch.full((B, P), -100, dtype=torch.int64), labels], dim=1)   # row i scored against label i
    nll, _ = R.row_scores(x.reshape(B * S, V), full.reshape(-1), V)
    loss = float(nll.sum()) / int((full >= 0).sum())
    assert abs(loss - float(g["loss"][0])) > 1e-3


def test_argmax_over_ld_and_last_maximum_are_told_apart():
    xt, yt = R.designed_targets(13, 16, torch.float32)
    _, hit = R.row_scores(xt, yt, 13)
    # over ld the padding columns (1e30 / NaN) take every argmax
    wrong_ld = R.first_argmax(xt.double()) == yt.long()
    assert hit.sum() >= 7 and wrong_ld.sum() == 0
    # the last maximum instead of the first flips the two tie rows
    x = xt[:, :13].double()
    last = 12 - R.first_argmax(torch.flip(x, dims=[1]))
    wrong_last = last == yt.long()
    assert bool(hit[2]) and not bool(hit[4]) and not bool(wrong_last[2]) and bool(wrong_last[4])


def test_designed_case_holds_its_conditions():
    for V, ld, dt in [(50257, 50304, torch.bfloat16), (512, 512, torch.float32), (13, 16, torch.bfloat16)]:
        xt, yt = R.designed_targets(V, ld, dt)
        nll, hit = R.row_scores(xt, yt, V)
        assert float(nll[R.NEG_INF_LABEL_ROW]) == float("inf") and math.isnan(float(nll[R.NAN_ROW]))
        assert torch.isfinite(nll).sum() == 13
        assert 6 <= int(hit.sum()) <= 9, hit           # the label is the maximum in about half of the rows
        assert bool(hit[2]) and not bool(hit[4])       # the two exact ties
        assert bool(torch.isinf(xt[6, :V].float()).any()) and bool(torch.isfinite(nll[6]))
        x, y, ranges = R.padded_layout(xt, yt)
        assert [int(((y[a:b]) >= 0).sum()) for a, b in zip(ranges[:-1], ranges[1:])] == list(R.SEQ_TARGETS)
        assert int((y >= 0).sum()) == 15
        for b, n in enumerate(R.SEQ_TARGETS):      # -100 rows interleaved: one between the first and last target
            t = torch.nonzero(y[12 * b: 12 * b + 12] >= 0).reshape(-1)
            assert n < 2 or int(t[-1] - t[0]) + 1 > n


# -------------------------------------------------------------------------------------------------- argument rules

def test_labels_from_mask():
    from icap.models import labels_from_mask

    ids = torch.tensor([[5, 6, 7, 8], [1, 2, 3, 4]])
    mask = torch.tensor([[1, 1, 0, 0], [1, 1, 1, 1]])
    assert labels_from_mask(ids, mask).tolist() == [[5, 6, -100, -100], [1, 2, 3, 4]]
    out = labels_from_mask(ids.to(torch.int32))
    assert out.dtype == torch.int64 and out.tolist() == ids.tolist()


@pytest.mark.parametrize("kw", [dict(select_by="val_loss"), dict(select_by="bleu"),
                                dict(eval_loss=True, select_by="nope")])
def test_train_rejects_bad_selection_before_any_work(kw, tmp_path):
    import icap

    out = tmp_path / "never_made"
    with pytest.raises(ValueError, match="select_by"):
        icap.train(None, None, batch_size=2, num_epochs=1, outputs_dir=str(out), **kw)
    with pytest.raises(ValueError, match="select_by"):
        icap.train_rat(None, None, None, 2, 2, batch_size=2, num_epochs=1, outputs_dir=str(out), **kw)
    assert not out.exists()


def test_train_defaults_return_the_same_keys(tmp_path):
    import icap
    import icap.weights
    from dryrun import dry_run
    from icap.dataset import SyntheticCaptionDataset
    from test_dryrun_bounds import tiny_model

    ds = SyntheticCaptionDataset(4, max_length=12, real=5, vocab_size=512, eos=511, embed_dim=64)
    with dry_run() as rec:
        icap.weights.ops.call = rec
        out = icap.train(ds, tiny_model(), batch_size=2, num_epochs=1, num_workers=0, device=torch.device("cpu"),
                         outputs_dir=str(tmp_path), save_every_epoch=10, use_graph=False)
    assert set(out) == {"epoch_losses", "val_metrics", "best_val_cider", "best_epoch"}
    assert out["val_metrics"] == [] and out["best_val_cider"] == -1.0 and out["best_epoch"] == 0
    assert not any(c[0].startswith("icap_caption_score") or c[0] == "icap_caption_target_ranges" for c in rec.calls)
    assert sorted(os.listdir(tmp_path)) == ["eval_results", "model_epoch_1.pt"]
