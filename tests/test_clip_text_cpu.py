"""CPU-only checks of the CLIP text tower: the torch restatement (tests/clip_text_helpers.py) against the goldens
transformers' CLIPModel produced (tools/make_clip_text_goldens.py), the pooled-position rule in both modes, the
HF key set, the argument rules, and the caption-embedding file the extraction functions write."""

import json
import os

import numpy as np
import pytest
import torch

import clip_text_helpers as H
import dryrun
from icap import (CLIPTextConfig, CLIPTextTower, build_retrieval_store, extract_caption_embeddings,
                  extract_clip_embedding_from_caption, get_image_id_from_filename, load_captions_annotations,
                  load_image_embeddings_file_names, map_caption_id_to_caption)

GEOMETRIES = {"clip_text_tiny": H.tiny_config, "clip_text_b32": H.b32_config}


@pytest.fixture(scope="module", params=sorted(GEOMETRIES))
def golden(request):
    cfg = GEOMETRIES[request.param]()
    g = dict(np.load(os.path.join(H.GOLD, request.param + ".npz")))
    return cfg, g, CLIPTextTower.random_init(cfg, seed=0).state_dict()


def test_golden_ids_regenerate(golden):
    cfg, g, _ = golden
    assert np.array_equal(g["ids"], H.golden_ids(cfg.vocab_size))
    assert int(g["eot"]) == cfg.vocab_size - 1
    lens = (g["pos_eos"] + 1).tolist()
    assert lens[:5] == [2, 3, 33, 65, 77] and lens[5] == 1  # the required lengths; the row without EOT pools 0
    assert (g["ids"][3, 65:] == g["eot"]).all()  # EOT-valued padding after the EOT
    assert not (g["ids"][5] == g["eot"]).any()


@pytest.mark.parametrize("mode", ["legacy", "eos"])
def test_pooled_positions_match_goldens(golden, mode):
    cfg, g, _ = golden
    eos = 2 if mode == "legacy" else int(g["eot"])
    assert np.array_equal(H.pooled_positions(g["ids"], eos), g["pos_" + mode])
    off, n, live = H.pack_ref(g["ids"], eos)
    assert np.array_equal(n, g["pos_" + mode] + 1) and live == int(n.sum())
    assert np.array_equal(off, np.cumsum(n) - n)
    assert g["pos_legacy"][5] == 11 and g["pos_eos"][5] == 0  # first maximum / no EOT


@pytest.mark.parametrize("mode", ["legacy", "eos"])
def test_restatement_matches_goldens(golden, mode):
    """fp32, every caption alone and unpadded: 1e-5 of transformers' padded batch (the bound of test_oracle.py)."""
    cfg, g, sd = golden
    eos = 2 if mode == "legacy" else int(g["eot"])
    f = H.text_features_ref(sd, cfg, g["ids"], eos)
    err = H.rel_err(f, torch.from_numpy(g["features_" + mode]))
    print(f"restatement vs transformers ({mode}): rel err {err:.3g}")
    assert err < 1e-5


def test_state_dict_keys_match_hf():
    want = json.load(open(os.path.join(H.GOLD, "clip_text_keys.json")))
    got = {k: list(v.shape) for k, v in CLIPTextTower().state_dict().items()}
    assert got == want
    assert not any(p.requires_grad for p in CLIPTextTower(H.tiny_config()).parameters())  # frozen


def test_config_defaults():
    c = CLIPTextConfig()
    assert (c.vocab_size, c.hidden_size, c.num_attention_heads, c.num_hidden_layers, c.intermediate_size,
            c.max_position_embeddings, c.projection_dim, c.eos_token_id, c.layer_norm_eps) == \
        (49408, 512, 8, 12, 2048, 77, 512, 2, 1e-5)
    l14 = CLIPTextConfig.vit_l14()
    assert (l14.hidden_size, l14.num_attention_heads, l14.intermediate_size, l14.projection_dim) == (768, 12, 3072, 768)
    assert l14.num_hidden_layers == 12 and l14.vocab_size == 49408


def test_argument_rules_and_no_fallback():
    """Ids outside the vocabulary raise ValueError whenever they are a host tensor; L above the position table
    raises; valid ids reach the missing device schedule, which is an error, never a host fallback."""
    from icap._lib import IcapError

    tower = CLIPTextTower(H.tiny_config())
    ids = torch.from_numpy(H.golden_ids(512))
    for bad in (512, -1):
        b = ids.clone()
        b[2, 5] = bad
        with pytest.raises(ValueError, match="vocabulary"):
            tower.get_text_features(b)
    with pytest.raises(ValueError, match="position table"):
        tower.get_text_features(torch.zeros((2, 78), dtype=torch.int64))
    for fn in (tower.get_text_features, tower.embed):
        with pytest.raises(IcapError, match="not part of this build"):
            fn(ids, attention_mask=torch.ones_like(ids))


def test_reference_helpers():
    assert get_image_id_from_filename("COCO_train2014_000000123456.jpg") == 123456
    anns = [{"image_id": i, "id": c, "caption": s} for i, c, s in H.CAPTIONS]
    m = map_caption_id_to_caption(anns)
    assert [c["caption_id"] for c in m[139]] == [11, 13, 16] and m[139][0]["caption"] == H.CAPTIONS[0][2]
    assert m.get(724, []) == []


def test_extract_caption_embeddings_file(tmp_path):
    """7 captions over 3 of 4 images, batch size 3, over the restated tower: the reference's file layout, filename
    order, first-seen grouping, un-normalised rows by default, and a file build_retrieval_store loads."""
    tower = CLIPTextTower.random_init(H.tiny_config(), seed=0)
    model, tok = H.RefTextModel(tower), H.StubTokenizer(512)
    img, ann = H.write_caption_fixture(tmp_path, D=64)
    assert load_image_embeddings_file_names(img) == H.IMAGE_FILES
    assert len(load_captions_annotations(ann)) == 7
    out = str(tmp_path / "captions.pt")
    assert extract_caption_embeddings(img, ann, out, model, tok, batch_size=3) == 7
    assert [c[0] for c in model.calls] == [3, 3, 1]  # three batches, each padded to its own maximum
    data = torch.load(out, weights_only=False)
    assert [d["filenames"] for d in data] == [H.IMAGE_FILES[0], H.IMAGE_FILES[1], H.IMAGE_FILES[3]]
    assert [[e["caption_id"] for e in d["embeddings"]] for d in data] == [[14, 17], [11, 13, 16], [12, 15]]
    order = [3, 6, 0, 2, 5, 1, 4]  # CAPTIONS rows in file order
    want = H.text_features_ref(tower.state_dict(), tower.config,
                               tok(text=[H.CAPTIONS[i][2] for i in order])["input_ids"].numpy())
    rows = []
    for d in data:
        assert set(d) == {"filenames", "embeddings"}
        for e in d["embeddings"]:
            assert set(e) == {"caption_id", "embedding"}
            assert isinstance(e["embedding"], np.ndarray) and e["embedding"].dtype == np.float32
            assert e["embedding"].shape == (64,)
            rows.append(torch.from_numpy(e["embedding"]))
    # padded per batch here, all together in `want`: the feature does not depend on the padded length
    assert H.rel_err(torch.stack(rows), want) < 1e-5
    assert float(torch.stack(rows).norm(dim=-1).sub(1).abs().min()) > 1e-3  # un-normalised, as the reference's batch path
    with dryrun.dry_run():  # (the store's device buffers on the host: nothing is launched by loading)
        store = build_retrieval_store(img, out, device=torch.device("cpu"))
        assert [m["caption_id"] for m in store.caption_metadata] == [14, 17, 11, 13, 16, 12, 15]
        assert torch.equal(store.caption_embeddings.cpu(), torch.stack(rows))
    extract_caption_embeddings(img, ann, out, model, tok, batch_size=7, normalize=True)
    unit = np.stack([e["embedding"] for d in torch.load(out, weights_only=False) for e in d["embeddings"]])
    assert np.abs(np.linalg.norm(unit.astype(np.float64), axis=1) - 1.0).max() < 1e-6
    one = extract_clip_embedding_from_caption(H.CAPTIONS[0][2], model, tok)
    assert one.shape == (64,) and abs(float(one.double().norm()) - 1.0) < 1e-6
