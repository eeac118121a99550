"""Retrieval kernels and the retrieval-augmented model on the GPU.

icap_topk_rows is compared exactly with a stable descending sort (values and indices; ties to the lower column).
icap_retrieval_aggregate and the store's pipeline are compared with the fp64 helper (tests/rat_helpers.py) on
stores whose scores satisfy the helper's two gap conditions, so the score GEMM's error decides nothing:
  cap_ids, retrieved and `max` bitwise; `mean` within (top_k + 1) 2^-23 and `sum_norm` within (top_k + D) 2^-23 of
  the row's max-abs (fp32 accumulation over that many terms).
The public classes are run on tests/golden/rat_tiny.npz (the reference's own outputs, tools/make_rat_goldens.py)
with the project's fp32 bounds: loss 2e-5, logits 1e-4 relative, greedy ids exact, train losses 1e-5 relative and
updates within 5 % of the largest update (tests/test_model_gpu.py).
"""

from types import SimpleNamespace

import numpy as np
import pytest
import torch

import rat_helpers as H
from icap import (DeviceRetrievalStore, GPT2Config, GPT2LMHeadModel, RetrievalAggregator,
                  RetrievalAugmentedTransformer, TransformerMappingNetwork, ops, train_rat)
from icap.dataset import SyntheticCaptionDataset
from oracle import icap_oracle as O

pytestmark = pytest.mark.gpu
S = ops.topk_rows_slice()
AGGS = ("mean", "max", "sum_norm")
TINY_G = O.GPT2Cfg(n_layer=2, n_embd=128, n_head=2, vocab_size=512, n_positions=128, eos=511)
TINY_M = O.MapperCfg(embed_dim=64, gpt_dim=128, prefix_length=5, hidden_length=4, num_layers=2)


# ------------------------------------------------------------------------------------------------- icap_topk_rows
def _rows(R, N, ld, gen):
    """Row kinds by r % 4: the maximum in the last column (the last, partial slice); few distinct values (many
    ties); all equal; plain random."""
    x = torch.randn((R, ld), generator=gen)
    for r in range(R):
        kind = r % 4
        if kind == 0:
            x[r, N - 1] = 10.0
        elif kind == 1:
            x[r] = torch.randint(0, 5, (ld,), generator=gen).float()
        elif kind == 2:
            x[r] = 0.25
    return x


def _ref_topk(x, K):
    R, N = x.shape
    s = torch.sort(x, dim=1, descending=True, stable=True)
    val = torch.full((R, K), float("-inf"), device=x.device)
    idx = torch.full((R, K), -1, dtype=torch.int32, device=x.device)
    val[:, : min(K, N)] = s.values[:, :K]
    idx[:, : min(K, N)] = s.indices[:, :K].int()
    return val, idx


def _topk(x, K, N, chunks=None):
    R = x.shape[0]
    tv = torch.full((R, K), 7.0, device=x.device)
    ti = torch.full((R, K), 7, dtype=torch.int32, device=x.device)
    ws = torch.empty(max(ops.topk_rows_workspace(R, N, K), 4) // 4, dtype=torch.int32, device=x.device)
    if chunks is None:
        ops.topk_rows(x, K, tv, ti, ws, N=N)
    else:
        for i, (c0, c1) in enumerate(zip(chunks[:-1], chunks[1:])):
            ops.topk_rows(x[:, c0:c1], K, tv, ti, ws, N=c1 - c0, col0=c0, merge=i > 0)
    return tv, ti


@pytest.mark.parametrize("K", [11, 14, 32])
@pytest.mark.parametrize("N", [1, 5, S - 1, S + 1, 2 * S + 3])
def test_topk_rows_exact(dev, N, K):
    gen = torch.Generator().manual_seed(N * 100 + K)
    for R in (1, 3, 130):
        for shift in range(4 if R == 1 else 1):  # a single row takes each kind in turn
            x = _rows(R + shift, N, N + 3, gen)[shift:].contiguous().to(dev)  # ld = N + 3 > N
            rv, ri = _ref_topk(x[:, :N], K)
            tv, ti = _topk(x, K, N)
            assert torch.equal(ti, ri), (R, shift)
            assert torch.equal(tv, rv), (R, shift)
            if N == 2 * S + 3:  # three column chunks folded into the running lists: bitwise the one-call lists
                cv, ci = _topk(x, K, N, chunks=[0, S + 1, S + 6, N])
                assert torch.equal(ci, ti) and torch.equal(cv, tv), (R, shift)


# --------------------------------------------------------------------------------------- stores with designed scores
def _orthonormal(n, D, gen):
    q, _ = torch.linalg.qr(torch.randn((D, n), generator=gen, dtype=torch.float64))
    return q.t().contiguous()  # n orthonormal rows


def _captions(N, top_k, D, gen):
    """Caption counts 0 ... 5 per image, one image with top_k + 3, one filename listed twice; rows shuffled so a
    file's rows are scattered; unit rows times a scale in [0.5, 2]."""
    counts = [[0, 1, 2, 3, 5, 4][n % 6] for n in range(N)]
    if N > 7:
        counts[7] = top_k + 3
    names = [f"img{n}.jpg" for n in range(N)]
    if N > 9:
        names[9] = names[2]
    owners = [names[n] for n in range(N) for _ in range(counts[n])]
    owners = [owners[int(i)] for i in torch.randperm(len(owners), generator=gen)]
    cap = torch.nn.functional.normalize(torch.randn((len(owners), D), generator=gen), dim=1)
    cap = cap * (0.5 + 1.5 * torch.rand((len(owners), 1), generator=gen))
    return names, owners, cap


def _designed(kind, B, D, top_i, top_k, gen):
    """(images [N, D], queries [B, D], names, caption owners, captions). Scores are designed: the images are
    orthonormal rows X and query b = sum_n w[b, n] X[n], so score(b, n) = w[b, n], a per-query shuffle of a grid
    with 0.01 steps below 0.95 plus, for `general`, up to two values above 1 (filtered like a self match).
    `small`: N = 5 < K. `filtered`: every image is the query times 1.001 + 0.001 n, so every score is above the
    threshold."""
    if kind == "filtered":
        N = 40
        q = torch.nn.functional.normalize(torch.randn(D, generator=gen, dtype=torch.float64), dim=0)
        images = q[None, :] * (1.001 + 0.001 * torch.arange(N, dtype=torch.float64))[:, None]
        queries = q[None, :].repeat(B, 1)
    else:
        N = 5 if kind == "small" else 48
        images = _orthonormal(N, D, gen)
        grid = 0.94 - 0.01 * torch.arange(N, dtype=torch.float64)
        w = torch.empty((B, N), dtype=torch.float64)
        for b in range(B):
            g = grid.clone()
            if kind == "general":
                g[: b % 3] = 1.02 + 0.01 * torch.arange(b % 3, dtype=torch.float64)
            w[b] = g[torch.randperm(N, generator=gen)]
        queries = w @ images
    names, owners, cap = _captions(N, top_k, D, gen)
    return images.float(), queries.float(), names, owners, cap


def _check_against_helper(dev, store, images, queries, names, owners, cap, top_i, top_k, D):
    lists = H.caption_lists(names, owners)
    scores, kept, ref_ids, ref_retr = H.retrieve(queries, images, cap, lists, top_i, top_k)
    assert H.conditions_hold(scores, top_i)
    B = queries.shape[0]
    q = queries.to(dev)
    ids = torch.empty((B, top_k), dtype=torch.int32, device=dev)
    retr = store.retrieve(q, top_i, top_k, cap_ids=ids)
    assert torch.equal(ids.cpu().long(), ref_ids)
    assert torch.equal(retr.cpu(), ref_retr)
    for agg in AGGS:
        ids.fill_(-7)
        out = store.augment(q, top_i, top_k, agg, cap_ids=ids).cpu()
        assert torch.equal(ids.cpu().long(), ref_ids), agg
        ref = H.aggregate(queries, ref_retr, agg)
        rowmax = ref.abs().max(dim=1, keepdim=True).values
        terms = {"mean": top_k + 1, "max": 0, "sum_norm": top_k + D}[agg]
        err = (out.double() - ref).abs()
        if agg == "max":
            assert torch.equal(out, ref.float()), agg
        else:
            assert bool((err <= terms * 2.0 ** -23 * rowmax).all()), (agg, float((err / rowmax).max()))
    return kept, ref_ids, ref_retr


def _store_of(dev, images, names, owners, cap, **kw):
    meta = [{"filename": f, "caption_id": i} for i, f in enumerate(owners)]
    return DeviceRetrievalStore(images, cap, names, meta, dev, **kw)


@pytest.mark.parametrize("top_i,top_k", [(1, 1), (4, 10), (6, 20), (22, 64)])
@pytest.mark.parametrize("B", [1, 3, 130])
@pytest.mark.parametrize("D", [64, 512])
def test_retrieval_aggregate_matches_helper(dev, D, B, top_i, top_k):
    gen = torch.Generator().manual_seed(D + 7 * B + top_k)
    for kind in ("general", "small", "filtered"):
        images, queries, names, owners, cap = _designed(kind, B, D, top_i, top_k, gen)
        store = _store_of(dev, images, names, owners, cap)
        kept, ids, retr = _check_against_helper(dev, store, images, queries, names, owners, cap, top_i, top_k, D)
        if kind == "filtered":  # everything filtered: nothing kept, all zeros, out = query
            assert bool((kept == -1).all()) and bool((ids == -1).all()) and not retr.any()
            assert torch.equal(store.augment(queries.to(dev), top_i, top_k, "mean").cpu(), queries)
        if kind == "small":
            assert store.num_images < top_i + 10
        if kind == "general":
            lists = H.caption_lists(names, owners)
            assert any(not l for l in lists) and len(lists[7]) > top_k


def test_score_cap_chunks_equal_one_chunk(dev):
    """max_score_bytes forced small: 48 images in three chunks of 16 columns give bitwise the unchunked result."""
    gen = torch.Generator().manual_seed(5)
    B, D, top_i, top_k = 3, 64, 4, 10
    images, queries, names, owners, cap = _designed("general", B, D, top_i, top_k, gen)
    one = _store_of(dev, images, names, owners, cap)
    three = _store_of(dev, images, names, owners, cap, max_score_bytes=4 * B * 16)
    assert one.chunk_columns(B) == 48 and three.chunk_columns(B) == 16
    q = queries.to(dev)
    for agg in AGGS:
        i1 = torch.empty((B, top_k), dtype=torch.int32, device=dev)
        i3 = torch.empty_like(i1)
        a, b = one.augment(q, top_i, top_k, agg, cap_ids=i1), three.augment(q, top_i, top_k, agg, cap_ids=i3)
        assert torch.equal(a, b) and torch.equal(i1, i3), agg
    v1, x1 = one.search(q, 14)
    v3, x3 = three.search(q, 14)
    assert torch.equal(x1, x3) and torch.equal(v1, v3)


# ------------------------------------------------------------------------------------------ the reference's golden
@pytest.fixture(scope="module")
def gold():
    return H.load_golden()


def _gold_store(g, dev):
    return DeviceRetrievalStore(g["image_embeddings"], g["caption_embeddings"], g["image_filenames"],
                                g["caption_metadata"], dev)


def _build_rat(dtype, dev, agg="mean", gc=TINY_G, mc=TINY_M):
    gpt = GPT2LMHeadModel(GPT2Config(vocab_size=gc.vocab_size, n_positions=gc.n_positions, n_embd=gc.n_embd,
                                     n_layer=gc.n_layer, n_head=gc.n_head, layer_norm_epsilon=gc.eps,
                                     eos_token_id=gc.eos))
    missing, unexpected = gpt.load_state_dict(O.gpt2_state_dict(gc, 0), strict=False)
    assert not unexpected and missing == ["lm_head.weight"]
    m = TransformerMappingNetwork(mc.embed_dim, mc.gpt_dim, mc.prefix_length, mc.hidden_length, mc.num_layers)
    m.load_state_dict(O.mapper_state_dict(mc, 0))
    model = RetrievalAugmentedTransformer(mc.embed_dim, 4, agg, m, tokenizer=SimpleNamespace(eos_token_id=gc.eos),
                                          gpt=gpt, freeze_gpt_weights=True, compute_dtype=dtype)
    return model.to(dev)


def _rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def test_golden_retrieve_and_augment(dev, gold):
    """_retrieve_batch bitwise; augment per aggregation type: `max` bitwise, `mean` / `sum_norm` (two fp32
    summations in different orders) within the accumulation bounds of the module docstring; the aggregator class on
    the golden's retrieved rows gives bitwise what augment gives."""
    assert H.conditions_hold(gold["scores"], gold["top_i"])
    store = _gold_store(gold, dev)
    top_i, top_k = gold["top_i"], gold["top_k"]
    q = torch.from_numpy(gold["queries"]).to(dev)
    ids = torch.empty((6, top_k), dtype=torch.int32, device=dev)
    assert np.array_equal(store.retrieve(q, top_i, top_k, cap_ids=ids).cpu().numpy(), gold["retrieved"])
    assert np.array_equal(ids.cpu().numpy(), gold["cap_ids"])
    tv, ti = store.search(q, top_i + 10)
    ref_scores = torch.from_numpy(gold["scores"])
    order = torch.sort(ref_scores, dim=1, descending=True, stable=True)
    assert torch.equal(ti.cpu().long(), order.indices[:, : top_i + 10])
    assert float((tv.cpu() - order.values[:, : top_i + 10]).abs().max()) <= 2e-6
    for agg in AGGS:
        model = _build_rat(torch.float32, dev, agg)
        assert torch.equal(model._retrieve_batch(store, q, top_i, top_k).cpu(), torch.from_numpy(gold["retrieved"]))
        out = model.augment(store, q, top_i, top_k)
        ref = torch.from_numpy(gold["augmented_" + agg])
        err = (out.cpu().double() - ref.double()).abs()
        rowmax = ref.double().abs().max(dim=1, keepdim=True).values
        print(agg, "max |augment - golden| / rowmax", float((err / rowmax).max()))
        if agg == "max":
            assert torch.equal(out.cpu(), ref)
        else:
            terms = top_k + 1 if agg == "mean" else top_k + 64
            assert bool((err <= terms * 2.0 ** -23 * rowmax).all()), agg
        again = RetrievalAggregator(64, agg)(q, torch.from_numpy(gold["retrieved"]).to(dev))
        assert torch.equal(again, out), agg


def test_golden_forward_and_greedy(dev, gold):
    store = _gold_store(gold, dev)
    model = _build_rat(torch.float32, dev).eval()
    ids, mask, labels, q = (torch.from_numpy(gold[k]).to(dev) for k in ("ids", "mask", "labels", "queries"))
    with torch.no_grad():
        out = model(store, gold["top_i"], gold["top_k"], ids, q, mask, labels)
    print("loss", out.loss.item(), "golden", gold["loss"][0], "logits rel", _rel(out.logits, gold["logits"]))
    assert abs(out.loss.item() - gold["loss"][0]) < 2e-5
    assert _rel(out.logits, gold["logits"]) < 1e-4
    gen = model.generate(store, gold["top_k"], gold["top_i"], q, max_length=20, temperature=0.0)
    assert np.array_equal(gen.cpu().numpy(), gold["greedy"])


class _ListDataset(torch.utils.data.Dataset):
    def __init__(self, ids, mask, labels, emb):
        self.t = (ids, mask, labels, emb)

    def __len__(self):
        return self.t[0].shape[0]

    def __getitem__(self, i):
        ids, mask, labels, emb = self.t
        return {"token_ids": ids[i], "labels": labels[i], "image_embedding": emb[i], "attention_mask": mask[i],
                "caption_text": "", "image_id": i}


def test_golden_train_rat_two_steps(dev, gold, tmp_path):
    """Two train_rat steps (one batch per epoch, dropout off) against the reference's train_rat: losses to 1e-5
    relative, every recorded parameter's update within 5 % of its largest update (tests/test_model_gpu.py
    _check_updates). Tensors above 2^14 elements are recorded as rows [::4]."""
    store = _gold_store(gold, dev)
    model = _build_rat(torch.float32, dev)
    init = O.mapper_state_dict(TINY_M, 0)
    ds = _ListDataset(*(torch.from_numpy(gold[k]) for k in ("ids", "mask", "labels", "queries")))
    hist = train_rat(ds, model, store, gold["top_k"], gold["top_i"], batch_size=6, num_epochs=2, num_workers=0,
                     learning_rate=1e-4, save_every_epoch=10 ** 6, device=dev, outputs_dir=str(tmp_path),
                     dropout=False)
    print("train_rat losses", hist["epoch_losses"], "golden", gold["train_losses"])
    assert _rel(hist["epoch_losses"], gold["train_losses"]) < 1e-5
    for k, v in model.mapping_network.state_dict().items():
        v, i0 = v.detach().double().cpu(), init[k].double()
        if "trained_rows4." + k in gold:
            ref, v, i0 = torch.from_numpy(gold["trained_rows4." + k]).double(), v[::4], i0[::4]
        else:
            ref = torch.from_numpy(gold["trained." + k]).double()
        upd = (ref - i0).abs().max()
        assert (v - ref).abs().max() <= 0.05 * upd + 1e-7, k


# ------------------------------------------------------------------------------------------------ capture, bf16 run
def test_augment_captured_in_a_graph(dev):
    """augment inside a captured graph, replayed after the query buffer is overwritten, equals the eager call
    bitwise: the pipeline reads nothing back to the host."""
    gen = torch.Generator().manual_seed(11)
    B, D, top_i, top_k = 5, 64, 4, 10
    images, queries, names, owners, cap = _designed("general", 2 * B, D, top_i, top_k, gen)
    store = _store_of(dev, images, names, owners, cap)
    model = _build_rat(torch.float32, dev)
    q1, q2 = queries[:B].to(dev), queries[B:].to(dev)
    e1, e2 = model.augment(store, q1, top_i, top_k).clone(), model.augment(store, q2, top_i, top_k).clone()
    assert not torch.equal(e1, e2)
    q_buf, out_buf = q1.clone(), torch.zeros((B, D), device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with ops.graph_capture(g):
        model.augment(store, q_buf, top_i, top_k, out=out_buf)
    for q, e in ((q2, e2), (q1, e1)):
        q_buf.copy_(q)
        out_buf.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out_buf, e)


def test_train_rat_bf16_smoke(dev, tmp_path):
    gen = torch.Generator().manual_seed(3)
    N, D = 300, 64
    img = torch.nn.functional.normalize(torch.randn((N, D), generator=gen), dim=1)
    names = [f"{n}.jpg" for n in range(N)]
    owners = [names[int(i)] for i in torch.randint(0, N, (900,), generator=gen)]
    cap = torch.nn.functional.normalize(torch.randn((900, D), generator=gen), dim=1)
    store = _store_of(dev, img, names, owners, cap)
    model = _build_rat(torch.bfloat16, dev)
    before = {k: v.detach().clone() for k, v in model.mapping_network.state_dict().items()}
    ds = SyntheticCaptionDataset(8, max_length=12, real=5, vocab_size=512, eos=511, embed_dim=D)
    hist = train_rat(ds, model, store, 10, 4, batch_size=4, num_epochs=1, num_workers=0, device=dev,
                     outputs_dir=str(tmp_path), save_every_epoch=10 ** 6)
    assert len(hist["epoch_losses"]) == 1 and np.isfinite(hist["epoch_losses"][0])
    after = model.mapping_network.state_dict()
    assert any(not torch.equal(before[k], after[k]) for k in before)
    assert all(bool(torch.isfinite(v).all()) for v in after.values())
