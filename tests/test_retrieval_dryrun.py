"""CPU-only: the retrieval launches stay inside live allocations (tests/dryrun.py with extent models for the
retrieval entry points, restated from include/icap.h), through the store, the model and train_rat."""

import json
from types import SimpleNamespace

import pytest
import torch

import dryrun
import icap.weights
from icap import (DeviceRetrievalStore, GPT2Config, GPT2LMHeadModel, RetrievalAggregator,
                  RetrievalAugmentedTransformer, TransformerMappingNetwork, ops, train_rat)
from icap.dataset import SyntheticCaptionDataset

CPU = torch.device("cpu")


def _accesses(name, a):
    if name == "icap_topk_rows":
        R, N, scores, ld, K, _col0, _merge, tv, ti, ws, _s = a
        out = [("scores", scores, dryrun._rows(R, ld, N, 4)), ("top_val", tv, R * K * 4), ("top_idx", ti, R * K * 4),
               ("workspace", ws, ops.topk_rows_workspace(R, N, K))]
    elif name == "icap_retrieval_aggregate":
        B, D, K, _ti, top_k, _agg, tv, ti, N, ptr, rows, C_, cap, q, ldq, retr, ids, o, ldo, _s = a
        out = [("top_val", tv, B * K * 4), ("top_idx", ti, B * K * 4), ("cap_ptr", ptr, (N + 1) * 4),
               ("cap_rows", rows, 4), ("caption_embeddings", cap, C_ * D * 4), ("query", q, dryrun._rows(B, ldq, D, 4)),
               ("retrieved", retr, B * top_k * D * 4), ("cap_ids", ids, B * top_k * 4),
               ("out", o, dryrun._rows(B, ldo, D, 4))]
    else:
        return _orig_accesses(name, a)
    return [(lbl, int(p), int(n)) for lbl, p, n in out if p and n > 0]


_orig_accesses = dryrun.accesses


@pytest.fixture()
def rec(monkeypatch):
    monkeypatch.setattr(dryrun, "accesses", _accesses)
    # dry_run() itself swaps ops.call (icap.weights.ops is that module) and puts it back. Setting it again through
    # monkeypatch would make monkeypatch's later undo reinstall the recorder for every test that follows.
    assert icap.weights.ops is ops
    with dryrun.dry_run() as r:
        yield r


def _store(N=300, C=700, D=64, **kw):
    g = torch.Generator().manual_seed(0)
    names = [f"{n}.jpg" for n in range(N)]
    caps = [{"filename": names[int(i)], "caption_id": c}
            for c, i in enumerate(torch.randint(0, N, (C,), generator=g))]
    return DeviceRetrievalStore(torch.randn((N, D), generator=g), torch.randn((C, D), generator=g), names, caps, CPU,
                                **kw)


def _rat(dtype=torch.float32):
    gpt = GPT2LMHeadModel(GPT2Config(vocab_size=512, n_positions=128, n_embd=128, n_layer=2, n_head=2,
                                     eos_token_id=511))
    m = TransformerMappingNetwork(64, 128, 5, 4, 2)
    return RetrievalAugmentedTransformer(64, 4, "mean", m, tokenizer=SimpleNamespace(eos_token_id=511), gpt=gpt,
                                         compute_dtype=dtype)


def _clean(rec):
    assert rec.calls, "nothing recorded"
    bad = rec.check()
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("cap_bytes", [64 << 20, 4 * 7 * 128])  # one chunk / three chunks of 128 columns for B = 7
def test_store_launches_in_bounds(rec, cap_bytes):
    store = _store(max_score_bytes=cap_bytes)
    q = torch.randn(7, 64)
    for top_i, top_k in [(1, 1), (4, 10), (22, 64)]:
        ids = torch.empty((7, top_k), dtype=torch.int32)
        assert store.retrieve(q, top_i, top_k, cap_ids=ids).shape == (7, top_k, 64)
        for agg in ("mean", "max", "sum_norm"):
            assert store.augment(q, top_i, top_k, agg).shape == (7, 64)
    _clean(rec)
    topk = [c[1] for c in rec.calls if c[0] == "icap_topk_rows"]
    per_search = 1 if cap_bytes == 64 << 20 else 3
    assert len(topk) == 12 * per_search
    assert [c[6] for c in topk[:per_search]] == [0, 1, 1][:per_search]  # merge after the first chunk
    assert [c[5] for c in topk[:per_search]] == [0, 128, 256][:per_search]  # col0
    gemms = [c[1][0]._obj for c in rec.calls if c[0] == "icap_gemm"]
    assert all(g.split_k == 1 and g.in_dtype == 0 and g.c_dtype == 0 for g in gemms)


def test_model_and_aggregator_in_bounds(rec):
    store, model = _store(), _rat()
    emb = torch.randn(3, 64)
    ids = torch.randint(0, 500, (3, 12))
    with torch.no_grad():
        model.forward(store, 4, 10, ids, emb, torch.ones_like(ids), ids)
    model.generate(store, 10, 4, emb, max_length=6, temperature=0.0)
    RetrievalAggregator(64, "sum_norm")(emb, model._retrieve_batch(store, emb, 4, 10))
    _clean(rec)
    names = [c[0] for c in rec.calls]
    assert names.count("icap_retrieval_aggregate") == 4 and names.count("icap_topk_rows") == 3


def test_train_rat_in_bounds(rec, tmp_path):
    """Two epochs of 3 + 2 samples: one augment per batch into the batch size's buffer, then the fused step; the
    validation pass writes the reference's `_rat` files."""
    ds = SyntheticCaptionDataset(5, max_length=12, real=5, vocab_size=512, eos=511, embed_dim=64)
    ann = tmp_path / "ann.json"
    ann.write_text(json.dumps({"annotations": []}))
    hist = train_rat(ds, _rat(torch.bfloat16), _store(), 10, 4, batch_size=3, num_epochs=2, num_workers=0, device=CPU,
                     outputs_dir=str(tmp_path), save_every_epoch=10, use_graph=False, val_dataset=ds,
                     val_annotations_path=str(ann), eval_every_epoch=2, eval_max_length=4)
    _clean(rec)
    names = [c[0] for c in rec.calls]
    # 2 epochs x 2 training batches, then one validation pass of 2 batches through generate
    assert names.count("icap_retrieval_aggregate") == 6 and names.count("icap_adamw_step") == 4
    assert len(hist["epoch_losses"]) == 2 and [m["epoch"] for m in hist["val_metrics"]] == [2]
    assert (tmp_path / "model_epoch_2.pt").exists()
    preds = json.loads((tmp_path / "eval_results" / "epoch_2_val_predictions_rat.json").read_text())
    assert [p["image_id"] for p in preds] == [0, 1, 2, 3, 4]
    assert (tmp_path / "eval_results" / "epoch_2_val_metrics_rat.json").exists()
