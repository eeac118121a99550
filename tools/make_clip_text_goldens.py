"""Generate tests/golden/clip_text_{tiny,b32}.npz and clip_text_keys.json with transformers' own CLIPModel.

For each geometry, CLIPTextTower.random_init(cfg, seed=0).state_dict() (closed-form weights) is loaded into
transformers.CLIPModel (a minimal vision tower beside it: get_text_features never touches it) and
get_text_features(input_ids, attention_mask) is recorded in both pooling modes: config eos_token_id = 2 (the
openai checkpoints' legacy value: the pooled row is argmax(ids)) and eos_token_id = the EOT id (the first EOT).
Only inputs and outputs are stored: ids, pooled positions, features. clip_text_keys.json holds the text-tower key
names and shapes of transformers' default CLIPModel (the openai/clip-vit-base-patch32 geometry).

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/make_clip_text_goldens.py
"""

from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gpt2-image-captioning_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import clip_text_helpers as H  # noqa: E402
from icap import CLIPTextTower  # noqa: E402


def hf_model(cfg, eos_token_id: int):
    from transformers import CLIPConfig, CLIPModel

    text = dict(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers,
                num_attention_heads=cfg.num_attention_heads, intermediate_size=cfg.intermediate_size,
                max_position_embeddings=cfg.max_position_embeddings, layer_norm_eps=cfg.layer_norm_eps,
                hidden_act="quick_gelu", projection_dim=cfg.projection_dim, eos_token_id=eos_token_id,
                bos_token_id=cfg.vocab_size - 2, pad_token_id=0)
    vision = dict(hidden_size=32, num_hidden_layers=1, num_attention_heads=2, intermediate_size=32, image_size=32,
                  patch_size=16, projection_dim=cfg.projection_dim)
    model = CLIPModel(CLIPConfig(text_config=text, vision_config=vision, projection_dim=cfg.projection_dim)).eval()
    return model


def record(name: str, cfg) -> None:
    sd = CLIPTextTower.random_init(cfg, seed=0).state_dict()
    ids = H.golden_ids(cfg.vocab_size)
    eot = cfg.vocab_size - 1
    t_ids = torch.from_numpy(ids)
    mask = torch.zeros_like(t_ids)
    out = {"ids": ids, "eot": np.array(eot, np.int64)}
    for mode, eos in (("legacy", 2), ("eos", eot)):
        model = hf_model(cfg, eos)
        res = model.load_state_dict(sd, strict=False)
        assert not res.unexpected_keys, res.unexpected_keys
        assert all(not (k.startswith("text_model.") or k.startswith("text_projection")) for k in res.missing_keys), \
            res.missing_keys
        pos = H.pooled_positions(ids, eos)
        for b in range(ids.shape[0]):
            mask[b, :pos[b] + 1] = 1
        with torch.no_grad():
            f = model.get_text_features(input_ids=t_ids, attention_mask=mask)
            f = f if isinstance(f, torch.Tensor) else f.pooler_output
        out[f"pos_{mode}"] = pos
        out[f"features_{mode}"] = f.float().numpy()
    path = os.path.join(H.GOLD, name + ".npz")
    np.savez(path, **out)
    print(path, {k: v.shape for k, v in out.items()})


def record_keys() -> None:
    from transformers import CLIPConfig, CLIPModel

    with torch.device("meta"):
        model = CLIPModel(CLIPConfig())
    keys = {k: list(v.shape) for k, v in model.state_dict().items()
            if k.startswith("text_model.") or k == "text_projection.weight"}
    path = os.path.join(H.GOLD, "clip_text_keys.json")
    with open(path, "w") as f:
        json.dump(keys, f, indent=0, sort_keys=True)
        f.write("\n")
    print(path, len(keys), "keys")


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(16)
    record_keys()
    record("clip_text_tiny", H.tiny_config())
    record("clip_text_b32", H.b32_config())
