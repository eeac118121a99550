"""The CLIP text tower on the device (icap.clip_text.ClipTextCore): every GEMM plan its schedule can reach under
ROWS_CAP against fp64 (tests/golden/clip_text_plan_cover.json — before any run of the tower at those sizes), the
embedding / pooled-position kernel and the row gather, the tower against transformers' goldens and the torch
restatement (tests/clip_text_helpers.py), the independence of the result from padding, chunking, graph replay, the
out-of-vocabulary guard for device ids, and the caption-embedding file end to end.

Bounds. GEMM plans: |C - ref| / (|A| . |B|^T + |bias| + |resid|), the normalised error of tests/test_gemm_roles_gpu.py
and tests/test_kernels_gpu.py: 4e-3 for a bf16 C (1e-2 where K is split), 2e-6 for fp32 operands, 1e-5 for bf16
operands into an fp32 C. Tower: relative error < 1e-4 in fp32 and minimum cosine > 0.99 in bf16, the bounds
tests/test_parity_gpu.py holds the vision towers to."""

import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import clip_text_helpers as H
from icap import CLIPTextTower, build_retrieval_store, extract_caption_embeddings, ops
from icap import _lib as L
from icap.clip_text import CAPTIONS_CAP, ROWS_CAP, chunk_captions

pytestmark = pytest.mark.gpu

PLANS = json.load(open(os.path.join(H.GOLD, "clip_text_plan_cover.json")))["plans"]
CONFIGS = {"tiny": H.tiny_config, "b32": H.b32_config}
_towers = {}


def tower_of(geom, dev, mode="legacy"):
    """The seed-0 tower of a geometry on the device (built once), its pooling mode set for this call."""
    if geom not in _towers:
        t = CLIPTextTower.random_init(CONFIGS[geom](), seed=0)
        _towers[geom] = ({k: v.clone() for k, v in t.state_dict().items()}, t.to(dev))
    sd, t = _towers[geom]
    t.config.eos_token_id = 2 if mode == "legacy" else t.config.vocab_size - 1
    return sd, t


def golden(geom):
    return dict(np.load(os.path.join(H.GOLD, f"clip_text_{geom}.npz")))


def min_cos(a, b):
    return float(F.cosine_similarity(a.double().cpu(), b.double().cpu(), dim=-1).min())


# ------------------------------------------------------------------------------------------------ 1. plan cover

_operands = {}


def _host_rand(key, shape, scale):
    """Seeded fp32 host operand, made once per (role, shape) and never modified."""
    if (key, shape) not in _operands:
        g = torch.Generator().manual_seed(sum(map(ord, key)) + 31 * shape[0] + shape[-1])
        _operands[(key, shape)] = torch.randn(shape, generator=g) * scale
    return _operands[(key, shape)]


@pytest.mark.parametrize("p", PLANS, ids=[f"{p['geometry']}-{p['dtype']}-{p['kind']}-M{p['M']}" for p in PLANS])
def test_plan_cover_against_fp64(dev, p):
    """Each (GEMM kind, smallest M) of the cover file, with the tower's epilogue, through ops.gemm exactly as
    ClipTextCore.run calls it: the kernel the planner names is the one recorded, and the output matches the fp64
    product on the host."""
    M, N, K = p["M"], p["N"], p["K"]
    dt = torch.bfloat16 if p["dtype"] == "bf16" else torch.float32
    kind = p["kind"]
    cdt = torch.float32 if kind == "proj" else dt
    A = _host_rand("A", (ROWS_CAP, K), 1.0)[:M].to(dt)
    B = _host_rand("B", (N, K), 0.05).to(dt)
    bias = _host_rand("bias", (N,), 0.5) if kind != "proj" else None
    resid = _host_rand("resid", (ROWS_CAP, N), 1.0)[:M].to(dt) if kind in ("out", "fc2") else None
    act = L.ACT_QUICK_GELU if kind == "fc1" else L.ACT_NONE
    C = torch.full((M, N), float("nan"), dtype=cdt, device=dev)
    d = lambda t: None if t is None else t.to(dev)  # noqa: E731
    names = []

    class Rec:
        def launch(self, key, flops, fn):
            names.append(key[0])
            fn()

    ops.GEMM_TIMER = Rec()
    try:
        ops.gemm(d(A), d(B), C, bias=d(bias), act=act, resid=d(resid))
    finally:
        ops.GEMM_TIMER = None
    assert names == [p["name"]], names
    z = A.double() @ B.double().t()
    norm = (A.float().abs() @ B.float().abs().t()).double()
    if bias is not None:
        z += bias.double()
        norm += bias.double().abs()
    if act:
        z = z * torch.sigmoid(1.702 * z)
    if resid is not None:
        z += resid.double()
        norm += resid.double().abs()
    got = C.cpu().double()
    assert bool(torch.isfinite(got).all())
    err = float(((got - z).abs() / norm).max())
    tol = (1e-2 if p["splits"] > 1 else 4e-3) if cdt == torch.bfloat16 else 2e-6 if dt == torch.float32 else 1e-5
    print(f"{p['name']} splits {p['splits']} fused {p['fused']}: normalised err {err:.3g} (bound {tol:g})")
    assert err < tol, err


# ------------------------------------------------------------------------------------- 2. embed kernel, 3. gather


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("geom", ["tiny", "b32"])
@pytest.mark.parametrize("L_", [77, 1])
def test_embed_kernel(dev, geom, dtype, L_):
    """x = tok[ids] + pos, summed in fp32 and rounded once (fp32: the host sum bit for bit; bf16: its rounding), and
    pooled_row = b*L + pooled_positions in both modes — on the golden ids, which hold the row without EOT whose
    maximum repeats and the EOT-padded row."""
    sd, t = tower_of(geom, dev)
    c = t.config
    ids = torch.from_numpy(H.golden_ids(c.vocab_size)[:, :L_].copy())
    tok, pos = sd["text_model.embeddings.token_embedding.weight"], sd["text_model.embeddings.position_embedding.weight"]
    want = (tok[ids] + pos[:L_]).reshape(-1, c.hidden_size).to(dtype)
    B = ids.shape[0]
    core = t.core(dtype)
    for eos in (2, c.vocab_size - 1):
        x = torch.full((B * L_, c.hidden_size), float("nan"), dtype=dtype, device=dev)
        rows = torch.full((B,), -1, dtype=torch.int32, device=dev)
        oov = torch.zeros(1, dtype=torch.int32, device=dev)
        ops.clip_text_embed(ids.to(dev), core.tok, core.pos, eos, x, rows, oov)
        assert torch.equal(x.cpu(), want)
        assert rows.cpu().tolist() == (np.arange(B) * L_ + H.pooled_positions(ids.numpy(), eos)).tolist()
        assert int(oov.item()) == 0
    if L_ == 77:
        g = golden(geom)
        assert np.array_equal(H.pooled_positions(ids.numpy(), 2), g["pos_legacy"])
        assert np.array_equal(H.pooled_positions(ids.numpy(), c.vocab_size - 1), g["pos_eos"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rows_gather_bitwise(dev, dtype):
    g = golden("tiny")
    rows = (np.arange(6) * 77 + g["pos_legacy"]).astype(np.int32)
    rt = torch.from_numpy(rows).to(dev)
    s0 = _host_rand("g0", (6 * 77, 128), 1.0).to(dtype).to(dev)
    s1 = _host_rand("g1", (6 * 77, 128), 1.0).to(dtype).to(dev)
    d0, d1, d2 = (torch.full((6, 128), float("nan"), dtype=dtype, device=dev) for _ in range(3))
    ops.rows_gather(rt, s0, d0, s1, d1)
    ops.rows_gather(rt, s1, d2)  # one source
    idx = torch.from_numpy(rows.astype(np.int64)).to(dev)
    assert torch.equal(d0, s0[idx]) and torch.equal(d1, s1[idx]) and torch.equal(d2, s1[idx])
    # an index outside the source reads nothing: a zero row
    bad = rt.clone()
    bad[2], bad[4] = 6 * 77, -1
    ops.rows_gather(bad, s0, d0, s1, d1)
    assert not d0[2].any() and not d1[4].any() and torch.equal(d0[[0, 1, 3, 5]], s0[idx[[0, 1, 3, 5]]])


# -------------------------------------------------------------------------------------- 4. tower vs the goldens


@pytest.mark.parametrize("mode", ["legacy", "eos"])
@pytest.mark.parametrize("geom", ["tiny", "b32"])
def test_tower_matches_goldens(dev, geom, mode):
    """ids [6, 77] of the goldens against transformers' CLIPModel.get_text_features: fp32 rel err < 1e-4, bf16
    minimum cosine > 0.99. Measured (MI355X): see DESIGN.md, "CLIP text tower"."""
    _, t = tower_of(geom, dev, mode)
    g = golden(geom)
    want = torch.from_numpy(g["features_" + mode])
    ids = torch.from_numpy(g["ids"])
    f32 = t.get_text_features(ids.to(dev), attention_mask=torch.ones_like(ids), compute_dtype=torch.float32)
    assert f32.dtype == torch.float32 and f32.shape == want.shape and f32.device.type == "cuda"
    err = H.rel_err(f32, want)
    b16 = t.get_text_features(ids, compute_dtype=torch.bfloat16)  # host ids: checked on the host, copied over
    cos = min_cos(b16, want)
    print(f"{geom} {mode}: fp32 rel err {err:.3g}, bf16 min cosine {cos:.6f}")
    assert err < 1e-4
    assert cos > 0.99
    e = t.embed(ids.to(dev), compute_dtype=torch.float32)
    assert float((e.double().norm(dim=-1) - 1).abs().max()) < 1e-6
    assert H.rel_err(e, F.normalize(want.double(), dim=-1)) < 1e-4


# --------------------------------------------------------------------------------- 5. padding, 6. trimmed input


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("mode", ["legacy", "eos"])
def test_padding_cannot_reach_the_result(dev, mode, dtype):
    """Every id after each pooled position replaced by random ids that do not move it (legacy: below the row's
    maximum; eos: never the eos id): the same launches over independent rows, so the features are bitwise equal."""
    _, t = tower_of("tiny", dev, mode)
    V = t.config.vocab_size
    ids = H.golden_ids(V)
    eos = t.config.eos_token_id
    pos = H.pooled_positions(ids, eos)
    rng = np.random.RandomState(5)
    noisy = ids.copy()
    for b in range(ids.shape[0]):
        hi = int(ids[b].max()) if mode == "legacy" else V - 1  # exclusive: below the maximum / never eos
        n = ids.shape[1] - pos[b] - 1
        noisy[b, pos[b] + 1:] = rng.randint(0, hi, size=n)
    assert np.array_equal(H.pooled_positions(noisy, eos), pos) and not np.array_equal(noisy, ids)
    a = t.get_text_features(torch.from_numpy(ids).to(dev), compute_dtype=dtype)
    b_ = t.get_text_features(torch.from_numpy(noisy).to(dev), compute_dtype=dtype)
    assert torch.equal(a, b_)


def test_trimmed_matches_padded(dev):
    """The golden captions of <= 33 tokens at L = 33 and at L = 77 (other launch extents, the same captions)."""
    _, t = tower_of("tiny", dev)
    g = golden("tiny")
    keep = [b for b in range(5) if H.LENGTHS[b] <= 33]
    assert keep == [0, 1, 2]
    ids = torch.from_numpy(g["ids"][keep])
    short = t.get_text_features(ids[:, :33].contiguous().to(dev), compute_dtype=torch.float32)
    full = t.get_text_features(ids.to(dev), compute_dtype=torch.float32)
    err = H.rel_err(short, full)
    print(f"L = 33 vs L = 77: rel err {err:.3g}")
    assert err < 1e-4
    assert H.rel_err(short, torch.from_numpy(g["features_legacy"][keep])) < 1e-4


# ------------------------------------------------------------------------------------------------ 7. at the cap


def _captions(B, L_, vocab, seed):
    """[B, L] ids: BOS, 1 ... L - 2 words, EOT, zero padding; caption 0 fills all L positions."""
    rng = np.random.RandomState(seed)
    ids = np.zeros((B, L_), dtype=np.int64)
    for b in range(B):
        n = L_ if b == 0 else rng.randint(3, L_ + 1)
        ids[b, 0] = vocab - 2
        ids[b, 1:n - 1] = rng.randint(3, vocab - 2, size=n - 2)
        ids[b, n - 1] = vocab - 1
    return ids


def test_tiny_at_the_cap_and_two_chunks(dev):
    sd, t = tower_of("tiny", dev)
    ids = _captions(300, 32, t.config.vocab_size, seed=1)
    assert chunk_captions(256, 32) == [(0, 256)] and 256 * 32 == ROWS_CAP and CAPTIONS_CAP == 256
    dids = torch.from_numpy(ids).to(dev)
    one = t.get_text_features(dids[:256], compute_dtype=torch.float32)
    assert bool(torch.isfinite(one).all())
    pick = list(range(0, 256, 17)) + [255]
    assert len(pick) == 16 + 1
    err = H.rel_err(one[pick], H.text_features_ref(sd, t.config, ids[pick]))
    print(f"tiny B = 256 L = 32, {len(pick)} sampled captions: rel err {err:.3g}")
    assert err < 1e-4
    # B = 300: two chunks (256 + 44), bitwise the two chunks run as calls of their own
    assert chunk_captions(300, 32) == [(0, 256), (256, 300)]
    both = t.get_text_features(dids, compute_dtype=torch.float32)
    tail = t.get_text_features(dids[256:], compute_dtype=torch.float32)
    assert torch.equal(both[:256], one) and torch.equal(both[256:], tail)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_b32_at_the_cap(dev, dtype):
    """One ViT-B/32-geometry chunk of ROWS_CAP token rows (every plan it launches ran in the cover test above):
    all finite, 8 sampled captions against the restatement."""
    sd, t = tower_of("b32", dev)
    ids = _captions(256, 32, t.config.vocab_size, seed=2)
    f = t.get_text_features(torch.from_numpy(ids).to(dev), compute_dtype=dtype)
    assert bool(torch.isfinite(f).all())
    pick = list(range(0, 256, 37)) + [255]
    assert len(pick) == 8
    want = H.text_features_ref(sd, t.config, ids[pick])
    if dtype == torch.float32:
        err = H.rel_err(f[pick], want)
        print(f"b32 B = 256 L = 32 fp32: rel err {err:.3g}")
        assert err < 1e-4
    else:
        cos = min_cos(f[pick], want)
        print(f"b32 B = 256 L = 32 bf16: min cosine {cos:.6f}")
        assert cos > 0.99


# -------------------------------------------------------------------------- 8. graph, 9. device ids out of range


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_graph_replay_matches_eager(dev, dtype):
    _, t = tower_of("tiny", dev)
    V = t.config.vocab_size
    first, second = torch.from_numpy(H.golden_ids(V, seed=0)).to(dev), torch.from_numpy(H.golden_ids(V, seed=3)).to(dev)
    assert not torch.equal(first, second)
    eager = [t.get_text_features(x, compute_dtype=dtype) for x in (first, second)]
    eager_emb = t.embed(second, compute_dtype=dtype)
    core = t.core(dtype)
    ws = core.alloc(6, 77)
    ws.ids.copy_(first)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with ops.graph_capture(g):
        core.run(ws, ws.ids)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(ws.feat32, eager[0])
    ws.ids.copy_(second)  # new ids into the static buffer
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(ws.feat32, eager[1]) and torch.equal(ws.emb, eager_emb)
    del g


def test_device_ids_outside_the_vocabulary(dev):
    """Ids that arrive as a device tensor cannot be checked on the host: the kernel reads no table row for an id
    outside [0, vocab) (zero token term), counts it, and get_text_features raises after reading the count back.
    The other captions of that call are what a clean call gives."""
    _, t = tower_of("tiny", dev)
    V = t.config.vocab_size
    ids = torch.from_numpy(H.golden_ids(V))
    clean = t.get_text_features(ids.to(dev), compute_dtype=torch.float32)
    bad = ids.clone()
    bad[2, 5] = V
    bad[2, 7] = -3
    for fn in (t.get_text_features, t.embed):
        with pytest.raises(ValueError, match="vocabulary"):
            fn(bad.to(dev), compute_dtype=torch.float32)
    with pytest.raises(ValueError, match="vocabulary"):
        t.get_text_features(bad)  # host ids: refused before anything runs
    # the schedule itself (what a captured graph replays) neither raises nor reads the count: the caller does
    core = t.core(torch.float32)
    ws = core.alloc(6, 77)
    ws.oov.zero_()
    core.run(ws, bad.to(dev))
    assert int(ws.oov.item()) == 2
    others = [0, 1, 3, 4, 5]
    assert torch.equal(ws.feat32[others], clean[others])
    assert bool(torch.isfinite(ws.feat32).all())
    assert torch.equal(t.get_text_features(ids.to(dev), compute_dtype=torch.float32), clean)  # the count was reset


# ----------------------------------------------------------------------------------------------- 10. end to end


def test_extract_caption_embeddings_on_device(dev, tmp_path):
    """extract_caption_embeddings over the device tower (fp32) and over the restatement: the same file."""
    _, t = tower_of("tiny", dev)
    host = CLIPTextTower.random_init(H.tiny_config(), seed=0)
    tok = H.StubTokenizer(512)
    img, ann = H.write_caption_fixture(tmp_path, D=64)

    class Fp32Tower:  # the extraction functions pass no compute dtype: pin fp32 for the parity bound
        device = t.device

        def get_text_features(self, input_ids, attention_mask=None):
            return t.get_text_features(input_ids, attention_mask, compute_dtype=torch.float32)

        def embed(self, input_ids, attention_mask=None):
            return t.embed(input_ids, attention_mask, compute_dtype=torch.float32)

    out_d, out_r = str(tmp_path / "device.pt"), str(tmp_path / "ref.pt")
    assert extract_caption_embeddings(img, ann, out_d, Fp32Tower(), tok, batch_size=3) == 7
    assert extract_caption_embeddings(img, ann, out_r, H.RefTextModel(host), tok, batch_size=3) == 7
    dd, rr = torch.load(out_d, weights_only=False), torch.load(out_r, weights_only=False)
    assert [x["filenames"] for x in dd] == [x["filenames"] for x in rr] == [H.IMAGE_FILES[i] for i in (0, 1, 3)]
    ids_d = [[e["caption_id"] for e in x["embeddings"]] for x in dd]
    assert ids_d == [[e["caption_id"] for e in x["embeddings"]] for x in rr] == [[14, 17], [11, 13, 16], [12, 15]]
    rows_d = torch.from_numpy(np.stack([e["embedding"] for x in dd for e in x["embeddings"]]))
    rows_r = torch.from_numpy(np.stack([e["embedding"] for x in rr for e in x["embeddings"]]))
    assert rows_d.dtype == torch.float32 and rows_d.shape == (7, 64)
    err = H.rel_err(rows_d, rows_r)
    print(f"caption file, device fp32 vs restatement: rel err {err:.3g}")
    assert err < 1e-4
    store = build_retrieval_store(img, out_d, device=dev)
    assert [m["caption_id"] for m in store.caption_metadata] == [14, 17, 11, 13, 16, 12, 15]
    assert torch.equal(store.caption_embeddings.cpu(), rows_d)
    # the tower as it is (bf16 by default) through the same function, normalised rows
    extract_caption_embeddings(img, ann, out_d, t, tok, batch_size=7, normalize=True)
    unit = np.stack([e["embedding"] for x in torch.load(out_d, weights_only=False) for e in x["embeddings"]])
    assert np.abs(np.linalg.norm(unit.astype(np.float64), axis=1) - 1.0).max() < 1e-6
    assert min_cos(torch.from_numpy(unit), rows_r) > 0.99
