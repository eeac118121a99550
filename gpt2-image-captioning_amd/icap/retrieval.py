"""DeviceRetrievalStore — the retrieval database of the retrieval-augmented captioner, resident on the device.

The reference keeps two FAISS indices on the host (src/database/faiss_store.py FAISSStore) and, in every forward,
copies the queries to the host, searches, walks a filename -> caption-rows dict, reconstructs the caption vectors
one by one and copies them back (src/models.py:655-695). Here the image and caption embeddings are device tensors,
the filename -> caption-rows dict is a CSR table, and a forward is the score GEMM S = Q . X^T (exact inner-product
search, the definition of faiss.IndexFlatIP; fp32 through icap_gemm) followed by icap_topk_rows and
icap_retrieval_aggregate (csrc/retrieval.hip): no host synchronisation, so it can be captured in a HIP graph.

Files: `build_retrieval_store` reads the two .pt files the reference's indexing pipeline reads
(src/database/faiss_indexing.py:49-113); `save_retrieval_store` / `create_retrieval_store` use one torch.save
file of our own; `DeviceRetrievalStore.from_faiss_store` converts a loaded FAISSStore (duck-typed).
"""

from __future__ import annotations

import os
import shutil
from typing import Optional

import torch

from . import _lib as L
from . import ops

Tensor = torch.Tensor

STORE_FILE = "retrieval_store.pt"
SEARCH_EXTRA = 10  # faiss_store.py:153 searches top_i + 10 candidates to leave room for the filter
MAX_TOP_I = 22     # K = top_i + 10 <= 32 (icap_topk_rows)
MAX_TOP_K = 64
# scores scratch [B, Nc] fp32: B = 128 queries against the 118 287 COCO train images (60.6 MB) in one chunk
DEFAULT_MAX_SCORE_BYTES = 64 << 20
AGG_CODES = {"mean": L.AGG_MEAN, "max": L.AGG_MAX, "sum_norm": L.AGG_SUM_NORM}


def check_limits(top_i: int, top_k: int) -> None:
    if not 1 <= int(top_i) <= MAX_TOP_I:
        raise ValueError(f"top_i must be in [1, {MAX_TOP_I}] (the search keeps top_i + {SEARCH_EXTRA} <= 32 "
                         f"candidates), got {top_i}")
    if not 1 <= int(top_k) <= MAX_TOP_K:
        raise ValueError(f"top_k must be in [1, {MAX_TOP_K}], got {top_k}")


def caption_csr(image_metadata, caption_metadata):
    """(cap_ptr int32 [N+1], cap_rows int32 [nnz]): for image n, cap_rows[cap_ptr[n]:cap_ptr[n+1]] are the caption
    rows of image_metadata[n]'s filename in the order FAISSStore.filename_to_caption_indices holds them
    (faiss_store.py:42-48). A filename without captions gets an empty range; a filename listed twice gets the same
    rows twice; captions of a filename that is not an image are reachable from no image."""
    by_name = {}
    for idx, meta in enumerate(caption_metadata):
        by_name.setdefault(meta["filename"], []).append(idx)
    ptr, rows = [0], []
    for name in image_metadata:
        rows.extend(by_name.get(name, ()))
        ptr.append(len(rows))
    if len(rows) >= 2 ** 31:
        raise ValueError("retrieval store: more than 2^31 - 1 (image, caption) pairs")
    return torch.tensor(ptr, dtype=torch.int32), torch.tensor(rows, dtype=torch.int32)


class DeviceRetrievalStore:
    """image_embeddings fp32 [N, D], caption_embeddings fp32 [C, D], cap_ptr / cap_rows (CSR, int32) on `device`;
    image_metadata (filenames) and caption_metadata (dicts with filename, caption_id) on the host, as FAISSStore.
    max_score_bytes caps the scores scratch [B, Nc]: above it the images are scored in column chunks whose top
    lists are folded into one (bitwise the same result)."""

    def __init__(self, image_embeddings: Tensor, caption_embeddings: Tensor, image_metadata, caption_metadata,
                 device=None, max_score_bytes: int = DEFAULT_MAX_SCORE_BYTES):
        device = torch.device(device if device is not None else "cuda")
        image_embeddings = torch.as_tensor(image_embeddings)
        caption_embeddings = torch.as_tensor(caption_embeddings)
        if image_embeddings.dim() != 2:
            raise ValueError("image_embeddings must be [N, D]")
        N, D = image_embeddings.shape
        if caption_embeddings.numel() == 0:
            caption_embeddings = caption_embeddings.reshape(0, D)
        if caption_embeddings.dim() != 2 or caption_embeddings.shape[1] != D:
            raise ValueError("caption_embeddings must be [C, D] with the images' D")
        if D % 4 != 0 or D == 0:
            raise ValueError(f"embedding dimension must be a positive multiple of 4, got {D}")
        if N >= 2 ** 31 or caption_embeddings.shape[0] >= 2 ** 31:
            raise ValueError("retrieval store: N and C must be below 2^31")
        self.image_metadata = list(image_metadata)
        self.caption_metadata = list(caption_metadata)
        if len(self.image_metadata) != N or len(self.caption_metadata) != caption_embeddings.shape[0]:
            raise ValueError("metadata lists must have one entry per embedding row")
        self.device = device
        self.image_embeddings = image_embeddings.to(device=device, dtype=torch.float32).contiguous()
        self.caption_embeddings = caption_embeddings.to(device=device, dtype=torch.float32).contiguous()
        ptr, rows = caption_csr(self.image_metadata, self.caption_metadata)
        self.cap_ptr, self.cap_rows = ptr.to(device), rows.to(device)
        self.max_score_bytes = int(max_score_bytes)
        self._scratch = {}

    # -- sizes ----------------------------------------------------------------------------------------------------
    @property
    def num_images(self) -> int:
        return self.image_embeddings.shape[0]

    @property
    def num_captions(self) -> int:
        return self.caption_embeddings.shape[0]

    @property
    def embed_dim(self) -> int:
        return self.image_embeddings.shape[1]

    def close(self) -> None:
        """API compatibility with FAISSStore.close."""

    @classmethod
    def from_faiss_store(cls, store, device=None, **kw) -> "DeviceRetrievalStore":
        """Convert a loaded FAISSStore (or anything shaped like one): needs image_index / caption_index with
        `ntotal` and `reconstruct_n(0, n)`, and the two metadata lists."""
        def vectors(index):
            n = int(index.ntotal)
            if n == 0:
                return torch.zeros((0, int(index.d)), dtype=torch.float32)
            return torch.as_tensor(index.reconstruct_n(0, n), dtype=torch.float32)

        return cls(vectors(store.image_index), vectors(store.caption_index), store.image_metadata,
                   store.caption_metadata, device, **kw)

    # -- device pipeline --------------------------------------------------------------------------------------------
    def chunk_columns(self, B: int) -> int:
        """Image columns scored per GEMM for B queries under max_score_bytes."""
        return max(1, min(max(self.num_images, 1), self.max_score_bytes // (4 * max(B, 1))))

    def _buffers(self, B: int, K: int):
        key = (B, K, self.max_score_bytes)
        s = self._scratch.get(key)
        if s is None:
            dev, cols = self.device, self.chunk_columns(B)
            s = {"scores": torch.empty(B * cols, dtype=torch.float32, device=dev),
                 "top_val": torch.empty((B, K), dtype=torch.float32, device=dev),
                 "top_idx": torch.empty((B, K), dtype=torch.int32, device=dev),
                 "ws": torch.empty(max(ops.topk_rows_workspace(B, cols, K), 8) // 4, dtype=torch.int32, device=dev)}
            self._scratch[key] = s
        return s

    def _query(self, image_embeddings: Tensor) -> Tensor:
        q = image_embeddings.to(device=self.device, dtype=torch.float32).contiguous()
        if q.dim() != 2 or q.shape[1] != self.embed_dim:
            raise ValueError(f"queries must be [B, {self.embed_dim}], got {tuple(image_embeddings.shape)}")
        return q

    def search(self, q: Tensor, K: int):
        """IndexFlatIP.search(q, K) on the device: (top_val fp32 [B, K], top_idx int32 [B, K]), descending, ties to
        the lower image index, index -1 past num_images entries. The returned tensors are this store's scratch for
        (B, K): the next search with the same sizes overwrites them."""
        L.require_device(self.device)
        B, N = q.shape[0], self.num_images
        s = self._buffers(B, K)
        cols = self.chunk_columns(B)
        for i, c0 in enumerate(range(0, max(N, 1), cols)):
            nc = min(cols, N - c0)
            view = s["scores"][: B * nc].view(B, nc)
            if nc and B:
                # split_k = 1: every score is one unsplit K chain whatever the chunk's width
                ops.gemm(q, self.image_embeddings[c0:c0 + nc], view, split_k=1)
            ops.topk_rows(view, K, s["top_val"], s["top_idx"], s["ws"], N=nc, col0=c0, merge=i > 0)
        return s["top_val"], s["top_idx"]

    def retrieve(self, image_embeddings: Tensor, top_i: int, top_k: int, *, cap_ids: Optional[Tensor] = None):
        """The reference's FAISS branch of _retrieve_batch (src/models.py:675-695): fp32 [B, top_k, D]."""
        check_limits(top_i, top_k)
        q = self._query(image_embeddings)
        tv, ti = self.search(q, top_i + SEARCH_EXTRA)
        out = torch.empty((q.shape[0], top_k, self.embed_dim), dtype=torch.float32, device=self.device)
        ops.retrieval_aggregate(tv, ti, self.cap_ptr, self.cap_rows, self.caption_embeddings, None, top_i=top_i,
                                top_k=top_k, agg=L.AGG_MEAN, retrieved=out, cap_ids=cap_ids)
        return out

    def augment(self, image_embeddings: Tensor, top_i: int, top_k: int, aggregation_type: str = "mean", *,
                out: Optional[Tensor] = None, cap_ids: Optional[Tensor] = None) -> Tensor:
        """query + aggregate(retrieved captions) as fp32 [B, D] (src/models.py:732-738) in four launches on the
        current stream; with `out` given nothing is allocated."""
        check_limits(top_i, top_k)
        if aggregation_type not in AGG_CODES:
            raise ValueError(f"Unknown aggregation_type: {aggregation_type}")
        q = self._query(image_embeddings)
        tv, ti = self.search(q, top_i + SEARCH_EXTRA)
        if out is None:
            out = torch.empty((q.shape[0], self.embed_dim), dtype=torch.float32, device=self.device)
        ops.retrieval_aggregate(tv, ti, self.cap_ptr, self.cap_rows, self.caption_embeddings, q, top_i=top_i,
                                top_k=top_k, agg=AGG_CODES[aggregation_type], cap_ids=cap_ids, out=out)
        return out


def build_retrieval_store(image_embedding_file_path: str, caption_embedding_file_path: str, device=None,
                          **kw) -> DeviceRetrievalStore:
    """The reference's indexing pipeline without FAISS (src/database/faiss_indexing.py:49-113): the image file holds
    {"embeddings": [N, D], "filenames": [...]}, the caption file a list of {"filenames": name, "embeddings":
    [{"embedding", "caption_id"}, ...]}; captions of an image that is not in the image file are skipped."""
    image_data = torch.load(image_embedding_file_path, weights_only=True)
    caption_data = torch.load(caption_embedding_file_path, weights_only=False)
    image_embeddings = image_data["embeddings"].to(torch.float32)
    filenames = list(image_data["filenames"])
    known = set(filenames)
    vectors, caption_metadata = [], []
    for entry in caption_data:
        name = entry["filenames"]
        if name not in known:
            continue
        for cap in entry["embeddings"]:
            vectors.append(torch.as_tensor(cap["embedding"], dtype=torch.float32).reshape(-1))
            caption_metadata.append({"filename": name, "caption_id": cap["caption_id"]})
    D = image_embeddings.shape[1]
    captions = torch.stack(vectors) if vectors else torch.zeros((0, D), dtype=torch.float32)
    return DeviceRetrievalStore(image_embeddings, captions, filenames, caption_metadata, device, **kw)


def save_retrieval_store(store: DeviceRetrievalStore, db_directory: str) -> None:
    os.makedirs(db_directory, exist_ok=True)
    torch.save({"format": 1, "image_embeddings": store.image_embeddings.cpu(),
                "caption_embeddings": store.caption_embeddings.cpu(), "image_metadata": store.image_metadata,
                "caption_metadata": store.caption_metadata}, os.path.join(db_directory, STORE_FILE))


def create_retrieval_store(db_directory: str, device=None, clear_db: bool = False,
                           **kw) -> Optional[DeviceRetrievalStore]:
    """Load a saved store. As create_faiss_store (faiss_store.py:70-92): clear_db on an existing directory empties
    it and returns None; a directory without the store file returns None."""
    if clear_db and os.path.exists(db_directory):
        shutil.rmtree(db_directory)
        os.makedirs(db_directory)
        return None
    path = os.path.join(db_directory, STORE_FILE)
    if not os.path.exists(path):
        return None
    d = torch.load(path, map_location="cpu", weights_only=True)
    return DeviceRetrievalStore(d["image_embeddings"], d["caption_embeddings"], d["image_metadata"],
                                d["caption_metadata"], device, **kw)
