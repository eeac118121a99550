"""CPU-only: the caption scorer's schedule (engine.CaptionScorer, evaluate.evaluate_loss, train(eval_loss=True)) run
under tests/dryrun.py — every recorded call's pointer extents lie inside live allocations. The extent models of the
two new entry points (icap_caption_score, icap_caption_target_ranges) live here, restated from include/icap.h, and
wrap dryrun.accesses, which has no model for them: a schedule from before that called them would raise there."""

import json
import os
from contextlib import contextmanager

import pytest
import torch

import dryrun
import icap
import icap.weights
from icap import CaptionScorer
from icap.dataset import SyntheticCaptionDataset
from test_dryrun_bounds import CPU, _assert_clean, batch, tiny_model

BACKWARD_BUFFERS = ("dx", "dx2", "dxd", "dff", "dqkv", "do", "da", "dhf", "d_emb")
NEW = ("icap_caption_score", "icap_caption_target_ranges")


def score_accesses(name, a):
    out = []
    if name == "icap_caption_score":
        (dt, rows, V, lg, ld, lab, rdev, B, rng, nll, ntok, ncor, tlp, P, Lc, slot, so, sl, tot, ws, _s) = a
        es = dryrun.ES[dt]
        out += [("logits", lg, dryrun._rows(rows, ld, V, es)), ("labels", lab, rows * 4), ("rows_dev", rdev, 4),
                ("ranges", rng, (B + 1) * 4), ("nll", nll, B * 4), ("n_tokens", ntok, B * 4),
                ("n_correct", ncor, B * 4), ("token_logprobs", tlp, B * Lc * 4), ("row_slot", slot, B * (P + Lc) * 4),
                ("seq_off", so, B * 4), ("seq_len", sl, B * 4), ("totals", tot, 24), ("workspace", ws, rows * 8)]
    elif name == "icap_caption_target_ranges":
        B, S, slot, so, sl, rng, _s = a
        out += [("row_slot", slot, B * S * 4), ("seq_off", so, B * 4), ("seq_len", sl, B * 4),
                ("ranges", rng, (B + 1) * 4)]
    return [(lbl, int(p), int(n)) for lbl, p, n in out if p and n > 0]


@contextmanager
def score_dry_run():
    orig = dryrun.accesses
    dryrun.accesses = lambda name, args: score_accesses(name, args) if name in NEW else orig(name, args)
    try:
        with dryrun.dry_run() as rec:
            icap.weights.ops.call = rec
            yield rec
    finally:
        dryrun.accesses = orig


def _names(rec):
    return [c[0] for c in rec.calls]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("form", ["padded", "compact", "packed"])
@pytest.mark.parametrize("mapper", ["transformer", "mlp"])
def test_scorer_in_bounds(mapper, form, dtype):
    """B = 3, P = 5, Lc = 12, V = 512: the padded grid, the compact head alone, packed rows + compact head."""
    with score_dry_run() as rec:
        model = tiny_model(mapper, dtype=dtype)
        sc = CaptionScorer(model, 3, 12, compact_head=form != "padded", pack_rows=form == "packed")
        assert (sc.gws.compact, sc.gws.pack) == (form != "padded", form == "packed")
        for name in BACKWARD_BUFFERS:
            assert not hasattr(sc.gws, name), name
        assert sc.gws.qdl is None
        ids, mask, labels, emb = batch(3, 12)
        sc.load_batch(ids, mask, labels, emb)
        n0 = len(rec.calls)
        sc.run(use_graph=False)
        _assert_clean(rec)
    names = _names(rec)[n0:]
    assert names[-2:] == ["icap_caption_target_ranges", "icap_caption_score"]
    assert names.count("icap_caption_score") == 1
    for gone in ("icap_cross_entropy", "icap_layernorm_bwd", "icap_attention_bwd", "icap_adamw_step",
                 "icap_counter_increment"):
        assert gone not in names, gone
    assert ("icap_caption_pack" in names) == (form == "packed")
    score = rec.calls[-1][1]
    assert score[1] == (3 * 12 if form != "padded" else 3 * 17) and score[2] == 512 and score[7] == 3
    assert (score[6] is not None) == (form != "padded") and (score[15] is not None) == (form != "padded")
    assert (score[16] is not None) == (form == "packed")
    # forward-only and dropout off: no launch carries a dropout probability
    for n, a in rec.calls[n0:]:
        if n == "icap_gemm":
            assert a[0]._obj.drop_p == 0.0
        if n == "icap_attention_fwd":
            assert a[0]._obj.drop_p == 0.0


def test_default_workspace_keeps_its_backward_buffers():
    with score_dry_run():
        model = tiny_model()
        ws = model._gcore().alloc_train(3, 5, 12, compact_head=True, pack=True)
        for name in BACKWARD_BUFFERS:
            assert isinstance(getattr(ws, name), torch.Tensor), name


def test_scorer_task_prefix_and_fp8_in_bounds():
    with score_dry_run() as rec:
        model = tiny_model(task_prompt="a photo of")
        sc = CaptionScorer(model, 4, 10)
        assert sc.P == 8
        sc.load_batch(*batch(4, 10))
        sc.run(use_graph=False)
        _assert_clean(rec)
    with score_dry_run() as rec:
        model = tiny_model(dtype=torch.bfloat16)
        model.gpt.fp8_mx = True
        sc = CaptionScorer(model, 3, 12)
        assert sc.gws.qhf is not None and sc.gws.qdl is None
        sc.load_batch(*batch(3, 12))
        sc.run(use_graph=False)
        _assert_clean(rec)
        assert "icap_quantize_mx" in _names(rec)


def test_short_sequence_flag_follows_the_host_labels():
    with score_dry_run():
        sc = CaptionScorer(tiny_model(), 3, 40)
        ids, mask, labels, emb = batch(3, 40)
        sc.load_batch(ids, mask, labels, emb)          # 5 + 20 tokens
        assert sc.gws.short_only is True
        labels = ids.clone()
        sc.load_batch(ids, torch.ones_like(mask), labels, emb)   # 5 + 40 tokens
        assert sc.gws.short_only is False


def test_existing_schedules_do_not_score():
    """The train step, forward and decode record none of the new entry points (dryrun.accesses itself would raise)."""
    with dryrun.dry_run() as rec:
        icap.weights.ops.call = rec
        model = tiny_model()
        t = icap.CaptionTrainer(model, 3, 12, num_training_steps=3)
        t.load_batch(*batch(3, 12))
        t.micro_step()
        ids, mask, labels, emb = batch(3, 12)
        with torch.no_grad():
            model(ids, emb, mask, labels)
        model.generate(emb, max_length=4, temperature=0.0)
    assert not set(NEW) & set(_names(rec))
    with pytest.raises(KeyError):
        dryrun.accesses("icap_caption_score", ())


def test_evaluate_loss_schedule(tmp_path):
    """10 captions in batches of 4: three scored batches, the short last one on a scorer of its own, all adding to
    one totals buffer; the result has the five keys."""
    from icap.evaluate import evaluate_loss

    ds = SyntheticCaptionDataset(10, max_length=12, real=5, vocab_size=512, eos=511, embed_dim=64)
    with score_dry_run() as rec:
        model = tiny_model()
        out = evaluate_loss(model, ds, batch_size=4, num_workers=0, device=CPU, use_graph=False)
        _assert_clean(rec)
    calls = [c[1] for c in rec.calls if c[0] == "icap_caption_score"]
    assert [c[7] for c in calls] == [4, 4, 2]
    assert len({c[18] for c in calls}) == 1           # one totals buffer
    assert set(out) == {"val_loss", "val_perplexity", "val_token_accuracy", "num_captions", "num_tokens"}
    assert out["num_captions"] == 10


def test_train_with_eval_loss_writes_the_keys(tmp_path):
    ds = SyntheticCaptionDataset(4, max_length=12, real=5, vocab_size=512, eos=511, embed_dim=64)
    with score_dry_run() as rec:
        out = icap.train(ds, tiny_model(), batch_size=2, num_epochs=1, num_workers=0, device=CPU,
                         outputs_dir=str(tmp_path), save_every_epoch=10, use_graph=False, val_dataset=ds,
                         val_annotations_path="unused.json", eval_max_length=4, eval_loss=True,
                         select_by="val_loss")
        _assert_clean(rec)
    assert set(out) == {"epoch_losses", "val_metrics", "best_val_cider", "best_epoch", "best_val_loss"}
    keys = {"epoch", "loss", "val_loss", "val_perplexity", "val_token_accuracy"}
    assert set(out["val_metrics"][0]) == keys
    with open(os.path.join(tmp_path, "eval_results", "val_metrics_summary.json")) as f:
        assert set(json.load(f)[0]) == keys
