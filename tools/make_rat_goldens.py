"""Generate tests/golden/rat_tiny.npz by running the REFERENCE's retrieval-augmented model (build container only).

As tools/make_goldens.py: the reference checkout (make_goldens.REF) is imported read-only and only inputs + outputs
are written. faiss is
not installed, so the reference's FAISSStore runs over a numpy stand-in of faiss.IndexFlatIP defined here (exact
inner-product search, descending, -1 padding: the index the reference's use_approximate=False builds). Everything
else is the reference's own code: FAISSStore, retrieve_images_by_vector_similarity, get_caption_embeddings,
RetrievalAggregator, RetrievalAugmentedTransformer.forward / .generate and train_rat.

One adaptation: RetrievalAugmentedTransformer._retrieve_batch passes embed_dim=512 to get_caption_embeddings
(src/models.py:690-692), which only sizes the zero padding; the fixture has D = 64, so the call is forwarded with
embed_dim=64.

The fixture is searched over seeds until the reference's own scores satisfy, for every query,
  - among the top top_i + 11 scores every gap is >= 1e-4,
  - no score lies within 1e-4 of the self-match threshold 0.9999 (none in the open interval (0.9998, 1.0)),
so a 2e-6 score error cannot change a decision, and until it contains every case listed in `scenarios`.

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/make_rat_goldens.py
"""

from __future__ import annotations

import os
import sys
import tempfile
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_goldens as MG  # noqa: E402
from make_goldens import O  # noqa: E402

D, N, B, TOP_I, TOP_K = 64, 40, 6, 4, 10
GAP = 1e-4
BIG = 1 << 14  # elements: trained tensors above it are recorded as rows [::4]
NO_CAPTIONS, MANY_CAPTIONS = 5, 7  # image rows: none / 12 captions


class IndexFlatIP:
    """The part of faiss.IndexFlatIP the reference uses."""

    def __init__(self, d):
        self.d = d
        self.x = np.zeros((0, d), dtype=np.float32)

    @property
    def ntotal(self):
        return self.x.shape[0]

    def add(self, v):
        self.x = np.concatenate([self.x, np.asarray(v, dtype=np.float32).reshape(-1, self.d)])

    def search(self, q, k):
        s = np.asarray(q, dtype=np.float32) @ self.x.T
        order = np.argsort(-s, axis=1, kind="stable")[:, :k]
        dist = np.full((s.shape[0], k), -np.inf, dtype=np.float32)
        idx = np.full((s.shape[0], k), -1, dtype=np.int64)
        dist[:, : order.shape[1]] = np.take_along_axis(s, order, 1)
        idx[:, : order.shape[1]] = order
        return dist, idx

    def reconstruct(self, i):
        return self.x[i].copy()

    def reconstruct_n(self, i0, n):
        return self.x[i0:i0 + n].copy()


def unit(x):
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)


def fixture(seed):
    rng = np.random.default_rng(seed)
    images = unit(rng.standard_normal((N, D)))
    counts = [[1, 2, 3, 4, 2, 5, 3][n % 7] for n in range(N)]
    counts[NO_CAPTIONS], counts[MANY_CAPTIONS] = 0, TOP_K + 2
    filenames = [f"img_{n:03d}.jpg" for n in range(N)]
    # caption rows interleaved across images, so a file's rows are not contiguous
    order = [n for r in range(max(counts)) for n in range(N) if r < counts[n]]
    cap_files = [filenames[n] for n in order]
    captions = unit(rng.standard_normal((len(order), D)))
    near = lambda n: unit(images[n] + 0.06 * rng.standard_normal(D))  # noqa: E731
    queries = np.stack([images[3], images[17], near(NO_CAPTIONS), near(MANY_CAPTIONS),
                        unit(rng.standard_normal(D)), unit(rng.standard_normal(D))])
    return images, filenames, captions, cap_files, queries


def conditions_hold(scores):
    """The band around the threshold is tested by its exact edges 0.9998 and 1.0: a self match scores exactly 1.0,
    at distance 1e-4, while the double nearest 0.9999 would put it at 9.9999999999989e-05."""
    s = scores.astype(np.float64)
    top = -np.sort(-s, axis=1)[:, : TOP_I + 11]
    return bool((top[:, :-1] - top[:, 1:]).min() >= GAP and not ((s > 0.9999 - GAP) & (s < 1.0)).any())


def main():
    MG.stub_modules()
    faiss = types.ModuleType("faiss")
    faiss.IndexFlatIP = IndexFlatIP
    faiss.Index = IndexFlatIP
    sys.modules["faiss"] = faiss
    sys.path.insert(0, MG.REF)
    import src.database.faiss_store as FS
    import src.models as RM
    import src.train as RT

    ref_gce = FS.get_caption_embeddings
    FS.get_caption_embeddings = lambda store, top_k, names, embed_dim=D: ref_gce(store, top_k, names, embed_dim=D)

    for seed in range(1000):
        images, filenames, captions, cap_files, queries = fixture(seed)
        image_index, caption_index = IndexFlatIP(D), IndexFlatIP(D)
        image_index.add(images)
        caption_index.add(captions)
        cap_meta = [{"filename": f, "caption_id": 1000 + i} for i, f in enumerate(cap_files)]
        store = FS.FAISSStore(image_index, caption_index, filenames, cap_meta)
        scores = queries @ images.T
        if not conditions_hold(scores):
            continue
        results = FS.retrieve_images_by_vector_similarity(store, queries, TOP_I)
        kept = np.full((B, TOP_I), -1, dtype=np.int64)
        for b, res in enumerate(results):
            kept[b, : len(res)] = [filenames.index(f) for f, _ in res]
        retrieved = FS.get_caption_embeddings(store, TOP_K, [[f for f, _ in res] for res in results])
        cap_ids = np.full((B, TOP_K), -1, dtype=np.int64)
        for b in range(B):
            for j in range(TOP_K):
                hit = np.flatnonzero((captions == retrieved[b, j]).all(axis=1))
                if np.any(retrieved[b, j]):
                    assert len(hit) == 1
                    cap_ids[b, j] = hit[0]
        n_caps = (cap_ids >= 0).sum(axis=1)
        used = [len({cap_files[c] for c in row if c >= 0}) for row in cap_ids]
        scenarios = {
            "self match dropped": 3 not in kept[0] and 17 not in kept[1] and scores[0, 3] > 0.9999,
            "image without captions kept": NO_CAPTIONS in kept[2],
            "more than top_k captions": kept[3, 0] == MANY_CAPTIONS and n_caps[3] == TOP_K,
            "padded": bool((n_caps < TOP_K).any()),
            "break before top_i images": any(u < (k >= 0).sum() for u, k, c in zip(used, kept, n_caps)
                                             if c == TOP_K),
        }
        if all(scenarios.values()):
            break
    else:
        raise SystemExit("no seed satisfies the fixture conditions")
    print("seed", seed, "captions", len(cap_files), "kept", kept.tolist(), "caption counts", n_caps.tolist())

    out = {"seed": np.array([seed]), "top_i": np.array([TOP_I]), "top_k": np.array([TOP_K]),
           "image_embeddings": images, "caption_embeddings": captions, "image_filenames": np.array(filenames),
           "caption_filenames": np.array(cap_files), "caption_ids": np.array([m["caption_id"] for m in cap_meta]),
           "queries": queries, "scores": scores.astype(np.float32), "kept_images": kept, "cap_ids": cap_ids,
           "retrieved": retrieved.astype(np.float32)}
    q_t, r_t = torch.from_numpy(queries), torch.from_numpy(retrieved)
    for agg in ("mean", "max", "sum_norm"):
        with torch.no_grad():
            out["augmented_" + agg] = RM.RetrievalAggregator(D, agg)(q_t, r_t).numpy()

    gcfg = O.GPT2Cfg(n_layer=2, n_embd=128, n_head=2, vocab_size=512, n_positions=128, eos=511)
    mcfg = O.MapperCfg(embed_dim=D, gpt_dim=128, prefix_length=5, hidden_length=4, num_layers=2)

    def build_rat():
        base, _, _ = MG.build_ref(gcfg, mcfg, seed=0)
        return RM.RetrievalAugmentedTransformer(D, 4, "mean", mapping_network=base.mapping_network,
                                                tokenizer=base.tokenizer, gpt=base.gpt, freeze_gpt_weights=True)

    ids, mask, labels, _ = O.synthetic_batch(B, 12, 7, gcfg.vocab_size, gcfg.eos, D, seed=1)
    out.update(ids=ids.numpy(), mask=mask.numpy(), labels=labels.numpy())
    torch.manual_seed(0)
    model = build_rat().eval()
    with torch.no_grad():
        assert torch.equal(model._retrieve_batch(store, q_t, TOP_I, TOP_K), r_t)
        res = model.forward(store, TOP_I, TOP_K, caption_token_ids=ids, image_embeddings=q_t, attention_mask=mask,
                            labels=labels)
        gen = model.generate(store, TOP_K, TOP_I, q_t, max_length=20, temperature=0.0)
    out["loss"] = np.array([res.loss.item()])
    out["logits"] = res.logits.numpy()
    out["logits_ck"] = MG.checksum(res.logits)
    out["greedy"] = gen.numpy()

    model = build_rat()
    with tempfile.TemporaryDirectory() as workdir:
        torch.manual_seed(0)
        hist = RT.train_rat(train_dataset=MG.ListDataset(ids, mask, labels, q_t), model=model, db_store=store,
                            top_k=TOP_K, top_i=TOP_I, batch_size=B, num_epochs=2, num_workers=0, learning_rate=1e-4,
                            num_warmup_steps=0, save_every_epoch=10 ** 6, device=torch.device("cpu"),
                            outputs_dir=os.path.join(workdir, "ckpt"))
    out["train_losses"] = np.array(hist["epoch_losses"])
    for k, v in model.mapping_network.state_dict().items():
        out["trained_ck." + k] = MG.checksum(v)
        # the file stays under 1 MiB: the large matrices are recorded as every fourth row
        if v.numel() > BIG:
            out["trained_rows4." + k] = v[::4].numpy()
        else:
            out["trained." + k] = v.numpy()
    path = os.path.join(MG.OUT, "rat_tiny.npz")
    np.savez_compressed(path, **out)
    print("rat_tiny loss", out["loss"], "train", out["train_losses"], "greedy", out["greedy"][0][:10],
          os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
