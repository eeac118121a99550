"""A plain-torch fp64 restatement of the retrieval-augmented embedding, shared by the retrieval tests:
exact inner-product search, the self-match filter, the caption walk, zero padding and the three aggregators
(the reference's src/database/faiss_store.py:132-251 and src/models.py:589-623, restated from their description in
include/icap.h; tests/golden/rat_tiny.npz holds the reference's own outputs).

Decisions (which images are kept, which caption rows are used) depend on score comparisons. They are robust to the
score GEMM's error (2e-6 for unit vectors, tests/test_kernels_gpu.py::test_gemm_plain) when, for every query,
  (a) among its top top_i + 11 scores every gap is >= 1e-4, and
  (b) no score lies within 1e-4 of the self-match threshold 0.9999,
which `conditions_hold` checks. (b) is tested by the band's exact edges, 0.9998 < s < 1.0: a self match scores
exactly 1.0, at distance 1e-4 in exact arithmetic, while the double nearest 0.9999 would put it at
9.9999999999989e-05.
"""

import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(__file__), "golden")
GAP = 1e-4
THRESHOLD = 0.9999
SEARCH_EXTRA = 10  # the reference searches top_i + 10 candidates


def load_golden():
    g = dict(np.load(os.path.join(GOLD, "rat_tiny.npz")))
    g["top_i"], g["top_k"] = int(g["top_i"][0]), int(g["top_k"][0])
    g["image_filenames"] = [str(x) for x in g["image_filenames"]]
    g["caption_filenames"] = [str(x) for x in g["caption_filenames"]]
    g["caption_metadata"] = [{"filename": f, "caption_id": int(c)}
                             for f, c in zip(g["caption_filenames"], g["caption_ids"])]
    return g


def conditions_hold(scores, top_i: int) -> bool:
    s = torch.as_tensor(scores).double()
    if s.shape[1] == 0:
        return True
    top = s.sort(dim=1, descending=True).values[:, : top_i + 11]
    gaps_ok = top.shape[1] < 2 or float((top[:, :-1] - top[:, 1:]).min()) >= GAP
    return bool(gaps_ok and not ((s > THRESHOLD - GAP) & (s < 1.0)).any())


def caption_lists(image_filenames, caption_filenames):
    """Per image row, the caption rows of its filename in caption order."""
    by_name = {}
    for i, f in enumerate(caption_filenames):
        by_name.setdefault(f, []).append(i)
    return [list(by_name.get(f, [])) for f in image_filenames]


def search(queries, images, K: int):
    """(scores fp64 [B, N], top values [B, K], top indices [B, K]): descending, ties to the lower index, the
    tail past N entries (-inf, -1)."""
    scores = torch.as_tensor(queries).double() @ torch.as_tensor(images).double().t()
    B, N = scores.shape
    order = torch.sort(scores, dim=1, descending=True, stable=True).indices[:, :K]
    val = torch.full((B, K), float("-inf"), dtype=torch.float64)
    idx = torch.full((B, K), -1, dtype=torch.int64)
    val[:, : order.shape[1]] = torch.gather(scores, 1, order)
    idx[:, : order.shape[1]] = order
    return scores, val, idx


def walk(val_row, idx_row, cap_lists, top_i: int, top_k: int):
    """(kept image rows, caption rows) of one query."""
    kept = []
    for v, i in zip(val_row.tolist(), idx_row.tolist()):
        if i == -1 or v > THRESHOLD:
            continue
        kept.append(i)
        if len(kept) >= top_i:
            break
    caps = []
    for i in kept:
        if cap_lists[i]:
            caps.extend(cap_lists[i])
            if len(caps) >= top_k:
                break
    return kept, caps[:top_k]


def retrieve(queries, images, captions, cap_lists, top_i: int, top_k: int):
    """scores fp64 [B, N], kept int64 [B, top_i] (-1 padded), cap_ids int64 [B, top_k] (-1 padded) and
    retrieved [B, top_k, D] in the captions' dtype (zero padded)."""
    captions = torch.as_tensor(captions)
    scores, val, idx = search(queries, images, top_i + SEARCH_EXTRA)
    B, D = scores.shape[0], captions.shape[1] if captions.dim() == 2 else torch.as_tensor(images).shape[1]
    kept = torch.full((B, top_i), -1, dtype=torch.int64)
    cap_ids = torch.full((B, top_k), -1, dtype=torch.int64)
    retrieved = torch.zeros((B, top_k, D), dtype=captions.dtype)
    for b in range(B):
        k, c = walk(val[b], idx[b], cap_lists, top_i, top_k)
        kept[b, : len(k)] = torch.tensor(k, dtype=torch.int64)
        cap_ids[b, : len(c)] = torch.tensor(c, dtype=torch.int64)
        if c:
            retrieved[b, : len(c)] = captions[torch.tensor(c)]
    return scores, kept, cap_ids, retrieved


def aggregate(query, retrieved, aggregation_type: str):
    """query + aggregate(retrieved) in fp64, zero pads taking part."""
    q, r = torch.as_tensor(query).double(), torch.as_tensor(retrieved).double()
    if aggregation_type == "mean":
        a = r.sum(dim=1) / r.shape[1]
    elif aggregation_type == "max":
        a = r.max(dim=1).values
    elif aggregation_type == "sum_norm":
        rn = r / r.norm(dim=2, keepdim=True).clamp_min(1e-12)
        s = rn.sum(dim=1)
        a = s / s.norm(dim=1, keepdim=True).clamp_min(1e-12)
    else:
        raise ValueError(aggregation_type)
    return q + a
