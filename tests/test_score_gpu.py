"""Caption scoring at model level on the tiny fixtures: ImageCaptioningModel.score_captions /
RetrievalAugmentedTransformer.score_captions / engine.CaptionScorer / evaluate.evaluate_loss / train(eval_loss=True).

fp32 parity mode against the restatement (tests/score_refs.py) applied to the REFERENCE's golden logits: per caption
|d nll| <= n_tokens * 2 * 1e-4 * max|golden logits| (the project's logits bound is 1e-4 relative to the largest logit;
a row's lse and its label logit each move by at most the largest logit error), the batch ratio within the existing
2e-5 of the golden loss. n_correct is compared where the oracle's top-two gap is >= 1e-3, and on these fixtures that
must be every target row. bf16: against the restatement applied to the logits the scorer itself produced (kernel
bounds), the batch ratio within test_model_gpu's 3e-2 of the golden loss."""

import functools
import glob
import os

import numpy as np
import pytest
import torch

import loss_refs
import rat_helpers as H
import score_refs as R
from icap import CaptionScorer
from icap.dataset import SyntheticCaptionDataset
from oracle import icap_oracle as O
from test_model_gpu import TINY_G, TINY_M, build, load
from test_retrieval_gpu import _build_rat, _gold_store

pytestmark = pytest.mark.gpu
P = 5
GAP = 1e-3
MLP_M = O.MLPMapperCfg(prefix_length=5, embed_dim=64, gpt_dim=128)


def _bound(ref, logits):
    return ref["n_tokens"].double() * 2 * 1e-4 * float(torch.as_tensor(logits).abs().max())


def _gaps_ok(logits, ys):
    """Every target row's top-two gap in these logits is >= GAP (a condition of the fixture, not a measurement)."""
    x = torch.as_tensor(logits).double().reshape(-1, logits.shape[-1])[ys.reshape(-1) >= 0]
    top = x.topk(2, dim=1).values
    gap = float((top[:, 0] - top[:, 1]).min())
    print("smallest top-two gap", gap)
    return gap >= GAP


def _check_against(out, ref, logits, labels):
    d = (out.nll.double().cpu() - ref["nll"]).abs()
    bound = _bound(ref, logits)
    print("per-caption |d nll|", d.tolist(), "bound", bound.tolist())
    assert bool((d <= bound).all())
    assert torch.equal(out.n_tokens.cpu().long(), ref["n_tokens"])
    assert _gaps_ok(logits, R.shifted_labels(labels, P))
    assert torch.equal(out.n_correct.cpu().long(), ref["n_correct"])
    assert torch.equal(out.logprob, -out.nll)
    tl = out.token_logprobs.cpu().double()
    assert torch.equal(tl == 0, torch.as_tensor(labels) == -100)
    assert float((tl - ref["token_logprobs"]).abs().max()) <= 2 * 1e-4 * float(torch.as_tensor(logits).abs().max())


@pytest.mark.parametrize("name", ["tiny", "tiny_mlp"])
def test_fp32_against_golden_logits(dev, name):
    g = load(name)
    model = (build(TINY_G, TINY_M, torch.float32, dev) if name == "tiny"
             else build(TINY_G, MLP_M, torch.float32, dev, mapper="mlp")).eval()
    ids, mask, labels, emb = (torch.from_numpy(g[k]) for k in ("ids", "mask", "labels", "emb"))
    out = model.score_captions(ids, emb, mask, labels, return_token_logprobs=True)
    ref = R.score(g["logits"], g["labels"], P)
    _check_against(out, ref, g["logits"], g["labels"])
    loss = float(out.nll.double().sum() / out.n_tokens.sum())
    print(name, "loss", loss, "golden", float(g["loss"][0]))
    assert abs(loss - float(g["loss"][0])) < 2e-5
    # labels=None: the ids where the mask is 1 — these fixtures' labels
    again = model.score_captions(ids, emb, mask)
    assert torch.equal(again.nll, out.nll) and not hasattr(again, "token_logprobs")


def test_fp32_rat_through_the_store(dev):
    g = H.load_golden()
    store = _gold_store(g, dev)
    model = _build_rat(torch.float32, dev).eval()
    ids, mask, labels, q = (torch.from_numpy(g[k]).to(dev) for k in ("ids", "mask", "labels", "queries"))
    out = model.score_captions(store, g["top_i"], g["top_k"], ids, q, mask, labels, return_token_logprobs=True)
    ref = R.score(g["logits"], g["labels"], P)
    _check_against(out, ref, g["logits"], g["labels"])
    loss = float(out.nll.double().sum() / out.n_tokens.sum())
    assert abs(loss - float(g["loss"][0])) < 2e-5


@functools.lru_cache(maxsize=None)
def _oracle_logits(case):
    """The tiny batch with its labels / mask cut (lengths 1, 4, 8; or caption 1 all ignored) and the CPU oracle's
    logits for it."""
    g = load("tiny")
    ids, mask, labels, emb = (torch.from_numpy(g[k]).clone() for k in ("ids", "mask", "labels", "emb"))
    if case == "lengths":
        for b, n in enumerate((1, 4, 8)):
            labels[b, n:] = -100
            mask[b, n:] = 0
    else:
        labels[1, :] = -100
    with torch.no_grad():
        prefix = O.mapper_forward(O.mapper_state_dict(TINY_M, 0), TINY_M, emb)
        _, logits = O.caption_forward(O.gpt2_state_dict(TINY_G, 0), TINY_G, prefix, ids, mask, labels)
    return ids, mask, labels, emb, logits


@pytest.mark.parametrize("case", ["lengths", "ignored"])
def test_unequal_lengths_packed_and_padded(dev, case):
    ids, mask, labels, emb, logits = _oracle_logits(case)
    ref = R.score(logits, labels, P)
    assert ref["n_tokens"].tolist() == ([1, 4, 8] if case == "lengths" else [8, 0, 8])
    model = build(TINY_G, TINY_M, torch.float32, dev).eval()
    outs = []
    for kw in (dict(), dict(compact_head=False, pack_rows=False)):
        sc = CaptionScorer(model, 3, 12, **kw)
        assert sc.gws.pack == (not kw)
        sc.load_batch(ids, mask, labels, emb)
        sc.run(use_graph=False)
        out = type("o", (), dict(nll=sc.nll.clone(), n_tokens=sc.n_tokens.clone(), n_correct=sc.n_correct.clone(),
                                 logprob=-sc.nll, token_logprobs=sc.token_logprobs.clone()))
        _check_against(out, ref, logits, labels)
        outs.append(out)
        t = sc.totals.cpu()
        assert t[1] == float(ref["n_tokens"].sum()) and t[2] == float(ref["n_correct"].sum())
    a, b = outs
    assert torch.equal(a.n_tokens, b.n_tokens) and torch.equal(a.n_correct, b.n_correct)
    assert bool(((a.nll - b.nll).abs().double().cpu() <= _bound(ref, logits)).all())
    if case == "ignored":
        assert float(a.nll[1]) == 0.0 and float(b.nll[1]) == 0.0


@pytest.mark.parametrize("form", ["padded", "packed"])
def test_bf16_against_its_own_logits(dev, form):
    g = load("tiny")
    ids, mask, labels, emb = (torch.from_numpy(g[k]) for k in ("ids", "mask", "labels", "emb"))
    model = build(TINY_G, TINY_M, torch.bfloat16, dev).eval()
    sc = CaptionScorer(model, 3, 12, compact_head=form == "packed", pack_rows=form == "packed")
    sc.load_batch(ids, mask, labels, emb)
    sc.run(use_graph=False)
    ws, V = sc.gws, 512
    assert ws.logits.dtype == torch.bfloat16
    if form == "padded":
        own = ws.logits.float().cpu().view(3, 17, -1)
        ref = R.score(own, labels, P, V=V)
        rows, ranges = ref["row_nll"].reshape(-1), [(b * 17, (b + 1) * 17) for b in range(3)]
        ntok, ncor, tlp = ref["n_tokens"], ref["n_correct"], ref["token_logprobs"]
    else:
        n = int(ws.n_valid.item())
        rg = sc.ranges.cpu().tolist()
        assert n == 24 and rg == [0, 8, 16, 24]
        rows, hit = R.row_scores(ws.logits[:n].float().cpu(), ws.labels_c[:n].cpu(), V)
        ranges = list(zip(rg[:-1], rg[1:]))
        ntok = torch.tensor([b - a for a, b in ranges])
        ncor = torch.stack([hit[a:b].sum() for a, b in ranges])
        tlp = torch.zeros((3, 12), dtype=torch.float64)
        tlp[labels != -100] = -rows
    seq_ratio = R.seq_ratio(sc.nll, rows, ranges)
    tl = sc.token_logprobs.cpu().double()
    row_ratio = loss_refs.loss_ratio(tl[labels != -100], tlp[labels != -100])
    print(form, "row ratio", row_ratio, "seq ratio", seq_ratio)
    assert row_ratio <= 1.0 and seq_ratio <= 1.0
    assert torch.equal(tl == 0, labels == -100)
    assert torch.equal(sc.n_tokens.cpu().long(), ntok.long()) and torch.equal(sc.n_correct.cpu().long(), ncor.long())
    loss = float(sc.totals[0] / sc.totals[1])
    print("bf16 loss", loss, "golden", float(g["loss"][0]))
    assert abs(loss - float(g["loss"][0])) < 3e-2


def _outputs(sc):
    return [t.clone() for t in (sc.nll, sc.n_tokens, sc.n_correct, sc.token_logprobs)]


def _same(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_graph_replay_equals_eager(dev, dtype):
    """A replay after the input buffers were overwritten equals the eager call bitwise; totals over three replays is
    the double sum of their fp32 nll and counts, bitwise; one graph per scorer."""
    ids, mask, labels, emb, _ = _oracle_logits("lengths")
    g = load("tiny")
    full = tuple(torch.from_numpy(g[k]) for k in ("ids", "mask", "labels", "emb"))
    cut = (ids, mask, labels, emb)
    model = build(TINY_G, TINY_M, dtype, dev).eval()
    sc = CaptionScorer(model, 3, 12)
    sc.load_batch(*cut)
    sc.run(use_graph=True)                      # the first call runs eagerly
    assert sc.graph is None
    eager_cut = _outputs(sc)
    sc.load_batch(*full)
    sc.run(use_graph=False)
    eager_full = _outputs(sc)
    assert not _same(eager_cut, eager_full)
    sc.reset()
    want = [0.0, 0.0, 0.0]
    for batch, eager in ((cut, eager_cut), (full, eager_full), (cut, eager_cut)):
        sc.load_batch(*batch)
        sc.run(use_graph=True)
        got = _outputs(sc)
        assert _same(got, eager)
        for b in range(3):
            want[0] += float(got[0][b])
            want[1] += float(got[1][b])
            want[2] += float(got[2][b])
    graph = sc.graph
    assert graph is not None
    t = sc.totals.cpu()
    assert torch.equal(t.view(torch.int64), torch.tensor(want, dtype=torch.float64).view(torch.int64)), (t, want)
    sc.load_batch(*full)
    sc.run(use_graph=True)
    assert sc.graph is graph


def test_evaluate_loss_short_last_batch(dev):
    from icap.evaluate import evaluate_loss

    ds = SyntheticCaptionDataset(10, max_length=12, real=5, vocab_size=512, eos=511, embed_dim=64)
    model = build(TINY_G, TINY_M, torch.float32, dev).eval()
    a = evaluate_loss(model, ds, batch_size=4, num_workers=0, device=dev)          # 4 + 4 + 2
    b = evaluate_loss(model, ds, batch_size=10, num_workers=0, device=dev)
    print(a, b)
    assert a["num_captions"] == b["num_captions"] == 10
    assert a["num_tokens"] == b["num_tokens"] == int((ds.labels != -100).sum())
    assert abs(a["val_loss"] - b["val_loss"]) <= 1e-6 * abs(b["val_loss"])
    assert abs(a["val_perplexity"] - np.exp(a["val_loss"])) <= 1e-9 * a["val_perplexity"]
    assert 0.0 <= a["val_token_accuracy"] <= 1.0
    # the batch route to the same number: forward()'s loss on all ten captions
    with torch.no_grad():
        out = model(ds.ids.to(dev), ds.emb.to(dev), ds.mask.to(dev), ds.labels.to(dev))
    assert abs(out.loss.item() - b["val_loss"]) < 2e-5


def test_train_selects_by_val_loss(dev, tmp_path):
    import icap

    tr = SyntheticCaptionDataset(8, max_length=12, real=5, vocab_size=512, eos=511, embed_dim=64)
    va = SyntheticCaptionDataset(6, max_length=12, real=5, vocab_size=512, eos=511, embed_dim=64, seed=2)
    model = build(TINY_G, TINY_M, torch.float32, dev)
    out = icap.train(tr, model, batch_size=4, num_epochs=2, num_workers=0, learning_rate=1e-3, device=dev,
                     outputs_dir=str(tmp_path), save_every_epoch=10, val_dataset=va,
                     val_annotations_path="no_metrics.json", eval_batch_size=4, eval_max_length=4, dropout=False,
                     eval_loss=True, select_by="val_loss")
    vm = out["val_metrics"]
    assert len(vm) == 2
    for m in vm:
        assert {"val_loss", "val_perplexity", "val_token_accuracy"} <= set(m) and np.isfinite(m["val_loss"])
    losses = [m["val_loss"] for m in vm]
    assert out["best_val_loss"] == min(losses)
    assert out["best_epoch"] == 1 + losses.index(min(losses))
    best = sorted(os.path.basename(p) for p in glob.glob(os.path.join(tmp_path, "best_model_epoch_*.pt")))
    assert f"best_model_epoch_{out['best_epoch']}.pt" in best and "best_model_epoch_1.pt" in best
