"""Retrieval store and argument rules that need no GPU: the fp64 helper against the reference's recorded outputs
(tests/golden/rat_tiny.npz, tools/make_rat_goldens.py), the CSR caption table, the store's files and the argument
checks of the retrieval-augmented model and train_rat."""

import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import rat_helpers as H
from icap import (DeviceRetrievalStore, GPT2Config, GPT2LMHeadModel, RetrievalAggregator,
                  RetrievalAugmentedTransformer, TransformerMappingNetwork, build_retrieval_store,
                  create_retrieval_store, save_retrieval_store, train_rat)
from icap.retrieval import caption_csr

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def gold():
    return H.load_golden()


def test_golden_fixture_conditions_and_cases(gold):
    """The recorded scores satisfy both gap conditions for every query, and the fixture holds every case."""
    top_i, top_k = gold["top_i"], gold["top_k"]
    assert gold["scores"].shape == (6, 40) and gold["queries"].shape == (6, 64)
    assert H.conditions_hold(gold["scores"], top_i)
    kept, cap_ids = gold["kept_images"], gold["cap_ids"]
    lists = H.caption_lists(gold["image_filenames"], gold["caption_filenames"])
    # queries 0 / 1 are database rows 3 / 17: the self match scores above the threshold and is dropped
    assert gold["scores"][0, 3] > 0.9999 and 3 not in kept[0]
    assert gold["scores"][1, 17] > 0.9999 and 17 not in kept[1]
    empty = [n for n, l in enumerate(lists) if not l]
    assert empty and any(n in kept for n in empty)  # an image without captions is among the kept ones
    big = [n for n, l in enumerate(lists) if len(l) > top_k]
    assert big and any(kept[b, 0] in big for b in range(6))  # an image with more than top_k captions comes first
    n_caps = (cap_ids >= 0).sum(axis=1)
    assert (n_caps < top_k).any()  # a padded query
    used = [len({gold["caption_filenames"][c] for c in row if c >= 0}) for row in cap_ids]
    assert any(n == top_k and u < (k >= 0).sum() for n, u, k in zip(n_caps, used, kept))  # break before top_i images


def test_helper_reproduces_golden(gold):
    lists = H.caption_lists(gold["image_filenames"], gold["caption_filenames"])
    scores, kept, cap_ids, retrieved = H.retrieve(gold["queries"], gold["image_embeddings"],
                                                  gold["caption_embeddings"], lists, gold["top_i"], gold["top_k"])
    assert float((scores - torch.from_numpy(gold["scores"]).double()).abs().max()) < 2e-6
    assert np.array_equal(kept.numpy(), gold["kept_images"])
    assert np.array_equal(cap_ids.numpy(), gold["cap_ids"])
    assert np.array_equal(retrieved.numpy(), gold["retrieved"])
    for agg in ("mean", "max", "sum_norm"):
        out = H.aggregate(gold["queries"], retrieved, agg)
        assert float((out - torch.from_numpy(gold["augmented_" + agg]).double()).abs().max()) < 1e-6, agg


def test_caption_csr_duplicates_empty_and_unknown():
    images = ["a.jpg", "b.jpg", "a.jpg", "c.jpg"]
    caps = [{"filename": f, "caption_id": i} for i, f in enumerate(["a.jpg", "zzz.jpg", "c.jpg", "a.jpg", "c.jpg"])]
    ptr, rows = caption_csr(images, caps)
    assert ptr.dtype == torch.int32 and rows.dtype == torch.int32
    assert ptr.tolist() == [0, 2, 2, 4, 6]  # b.jpg: empty range; both a.jpg rows: the same list
    assert rows.tolist() == [0, 3, 0, 3, 2, 4]  # caption 1 (zzz.jpg: not an image) is reachable from no image


def _fixture_files(tmp_path, D=8):
    g = torch.Generator().manual_seed(0)
    img = torch.nn.functional.normalize(torch.randn((3, D), generator=g), dim=1)
    cap = torch.nn.functional.normalize(torch.randn((5, D), generator=g), dim=1)
    ip, cp = str(tmp_path / "img.pt"), str(tmp_path / "cap.pt")
    torch.save({"embeddings": img, "filenames": ["a.jpg", "b.jpg", "c.jpg"]}, ip)
    torch.save([{"filenames": "c.jpg", "embeddings": [{"embedding": cap[0], "caption_id": 10},
                                                      {"embedding": cap[1].tolist(), "caption_id": 11}]},
                {"filenames": "missing.jpg", "embeddings": [{"embedding": cap[2], "caption_id": 12}]},
                {"filenames": "a.jpg", "embeddings": [{"embedding": cap[3], "caption_id": 13}]},
                {"filenames": "c.jpg", "embeddings": [{"embedding": cap[4], "caption_id": 14}]}], cp)
    return ip, cp, img, cap


def test_build_retrieval_store_skips_captions_of_absent_images(tmp_path):
    ip, cp, img, cap = _fixture_files(tmp_path)
    s = build_retrieval_store(ip, cp, CPU)
    assert (s.num_images, s.num_captions, s.embed_dim) == (3, 4, 8)
    assert torch.equal(s.image_embeddings, img) and torch.equal(s.caption_embeddings, cap[[0, 1, 3, 4]])
    assert s.image_metadata == ["a.jpg", "b.jpg", "c.jpg"]
    assert [m["caption_id"] for m in s.caption_metadata] == [10, 11, 13, 14]
    assert s.cap_ptr.tolist() == [0, 1, 1, 4] and s.cap_rows.tolist() == [2, 0, 1, 3]


def _same_store(a, b):
    return (torch.equal(a.image_embeddings, b.image_embeddings)
            and torch.equal(a.caption_embeddings, b.caption_embeddings) and torch.equal(a.cap_ptr, b.cap_ptr)
            and torch.equal(a.cap_rows, b.cap_rows) and a.image_metadata == b.image_metadata
            and a.caption_metadata == b.caption_metadata)


def test_store_save_and_create_round_trip(tmp_path):
    ip, cp, _, _ = _fixture_files(tmp_path)
    s = build_retrieval_store(ip, cp, CPU)
    db = str(tmp_path / "db")
    assert create_retrieval_store(db, CPU) is None  # missing directory
    save_retrieval_store(s, db)
    assert _same_store(create_retrieval_store(db, CPU), s)
    assert create_retrieval_store(db, CPU, clear_db=True) is None  # emptied, as create_faiss_store
    assert os.path.isdir(db) and os.listdir(db) == []
    assert create_retrieval_store(db, CPU) is None  # directory without the store file


def test_from_faiss_store_with_fake_index(gold):
    class FakeIndex:
        def __init__(self, x):
            self.x, self.ntotal, self.d = x, x.shape[0], x.shape[1]

        def reconstruct_n(self, i0, n):
            return self.x[i0:i0 + n].copy()

    fake = SimpleNamespace(image_index=FakeIndex(gold["image_embeddings"]),
                           caption_index=FakeIndex(gold["caption_embeddings"]),
                           image_metadata=gold["image_filenames"], caption_metadata=gold["caption_metadata"])
    s = DeviceRetrievalStore.from_faiss_store(fake, CPU)
    direct = DeviceRetrievalStore(gold["image_embeddings"], gold["caption_embeddings"], gold["image_filenames"],
                                  gold["caption_metadata"], CPU)
    assert _same_store(s, direct)
    lists = H.caption_lists(gold["image_filenames"], gold["caption_filenames"])
    ptr = s.cap_ptr.tolist()
    assert [s.cap_rows[ptr[n]:ptr[n + 1]].tolist() for n in range(s.num_images)] == lists


def test_store_rejects_bad_shapes():
    with pytest.raises(ValueError, match="multiple of 4"):
        DeviceRetrievalStore(torch.zeros(2, 6), torch.zeros(0, 6), ["a", "b"], [], CPU)
    with pytest.raises(ValueError, match="one entry per"):
        DeviceRetrievalStore(torch.zeros(2, 8), torch.zeros(0, 8), ["a"], [], CPU)


def _tiny_rat(aggregation_type="mean"):
    gpt = GPT2LMHeadModel(GPT2Config(vocab_size=64, n_positions=32, n_embd=32, n_layer=1, n_head=2, eos_token_id=63))
    m = TransformerMappingNetwork(8, 32, 2, 2, 1)
    return RetrievalAugmentedTransformer(8, 4, aggregation_type, m, tokenizer=SimpleNamespace(eos_token_id=63),
                                         gpt=gpt, compute_dtype=torch.float32)


def test_argument_rules(tmp_path):
    ip, cp, img, _ = _fixture_files(tmp_path)
    store = build_retrieval_store(ip, cp, CPU)
    model = _tiny_rat()
    assert isinstance(model.aggregator, RetrievalAggregator) and model.max_workers == 4
    assert not [k for k in model.state_dict() if k.startswith("aggregator")]  # checkpoint keys: the base class's
    for top_i, top_k in [(0, 10), (23, 10), (4, 0), (4, 65)]:
        with pytest.raises(ValueError, match="top_i|top_k"):
            model.augment(store, img, top_i, top_k)
        with pytest.raises(ValueError, match="top_i|top_k"):
            store.retrieve(img, top_i, top_k)
    foreign = SimpleNamespace(image_index=object())
    for call in (lambda: model.augment(foreign, img, 4, 10), lambda: model._retrieve_batch(foreign, img, 4, 10),
                 lambda: model.forward(foreign, 4, 10, torch.zeros((3, 4), dtype=torch.long), img),
                 lambda: model.generate(foreign, 10, 4, img)):
        with pytest.raises(TypeError, match="from_faiss_store"):
            call()
    with pytest.raises(NotImplementedError, match="attention"):
        RetrievalAggregator(8, "attention")
    with pytest.raises(NotImplementedError, match="attention"):
        _tiny_rat("attention")
    with pytest.raises(ValueError, match="Unknown aggregation_type: median"):
        RetrievalAggregator(8, "median")(img, torch.zeros(3, 2, 8))


def test_train_rat_argument_rules(tmp_path):
    ip, cp, _, _ = _fixture_files(tmp_path)
    store = build_retrieval_store(ip, cp, CPU)
    model = _tiny_rat()
    out = str(tmp_path / "ckpt")
    with pytest.raises(ValueError, match="val_annotations_path is required"):  # src/train.py:306-309
        train_rat([], model, store, 10, 4, 2, 1, outputs_dir=out, val_dataset=[])
    with pytest.raises(ValueError, match="clip_model"):
        train_rat([], model, store, 10, 4, 2, 1, outputs_dir=out, clip_model=object())
    with pytest.raises(TypeError, match="from_faiss_store"):
        train_rat([], model, SimpleNamespace(), 10, 4, 2, 1, outputs_dir=out)
    with pytest.raises(ValueError, match="top_i"):
        train_rat([], model, store, 10, 0, 2, 1, outputs_dir=out)
