"""CLIP text tower parameters and the caption-embedding file (src/embeddings/word_embeddings.py) — the host half.

`CLIPTextTower` holds the text half of HF CLIPModel under HF's own key names (text_model.*, text_projection.weight),
so an HF checkpoint loads directly, with a closed-form `random_init` whose outputs transformers' CLIPModel pins in
tests/golden/clip_text_*.npz (tools/make_clip_text_goldens.py). The extraction functions mirror the reference
(`extract_clip_embedding_from_caption` and the helpers of word_embeddings.py:11-82, and its `__main__` block :85-171
as `extract_caption_embeddings`) and write the structured caption file that `build_retrieval_store` reads.

The device schedule of the tower (HF/models/clip/modeling_clip.py: CLIPTextEmbeddings :221-256 -> 12 causal pre-LN
layers :353-384 -> final_layer_norm :559 -> the EOT row :561-582 -> text_projection :713) is not part of this
build: `CLIPTextTower.get_text_features` raises (there is no host fallback). The extraction functions take any
`clip_model` with `get_text_features` / `embed`, so they run today over another implementation of the tower and
over this one once its schedule is in ("CLIP text tower").
"""

from __future__ import annotations

import json
from collections import defaultdict
from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib as L
from .clip import _Encoder
from .weights import det_tensor

Tensor = torch.Tensor


@dataclass
class CLIPTextConfig:  # HF/models/clip/configuration_clip.py CLIPTextConfig (openai/clip-vit-base-patch32 values)
    vocab_size: int = 49408
    hidden_size: int = 512
    num_hidden_layers: int = 12
    num_attention_heads: int = 8
    intermediate_size: int = 2048
    max_position_embeddings: int = 77
    projection_dim: int = 512
    layer_norm_eps: float = 1e-5
    eos_token_id: int = 2  # the openai checkpoints' legacy value: the pooled row is argmax(ids)

    @classmethod
    def vit_l14(cls):  # openai/clip-vit-large-patch14
        return cls(hidden_size=768, num_attention_heads=12, intermediate_size=3072, projection_dim=768)


class _TextEmb(nn.Module):
    def __init__(self, c: CLIPTextConfig):
        super().__init__()
        self.token_embedding = nn.Embedding(c.vocab_size, c.hidden_size)
        self.position_embedding = nn.Embedding(c.max_position_embeddings, c.hidden_size)


class _TextModel(nn.Module):
    def __init__(self, c: CLIPTextConfig):
        super().__init__()
        self.embeddings = _TextEmb(c)
        self.encoder = _Encoder(c)
        self.final_layer_norm = nn.LayerNorm(c.hidden_size, eps=c.layer_norm_eps)


class CLIPTextTower(nn.Module):
    """The text half of HF CLIPModel (modeling_clip.py:683-715): parameter names and shapes are exactly HF's
    (tests/golden/clip_text_keys.json). Storage only, frozen."""

    def __init__(self, config: Optional[CLIPTextConfig] = None):
        super().__init__()
        self.config = config or CLIPTextConfig()
        self.text_model = _TextModel(self.config)
        self.text_projection = nn.Linear(self.config.hidden_size, self.config.projection_dim, bias=False)
        for p in self.parameters():
            p.requires_grad = False  # frozen encoder

    @classmethod
    def random_init(cls, config: Optional[CLIPTextConfig] = None, seed: int = 0) -> "CLIPTextTower":
        m = cls(config)
        c = m.config
        d = c.hidden_size
        t = "text_model."
        sd = {
            t + "embeddings.token_embedding.weight": det_tensor(seed, "t.tok", (c.vocab_size, d), 0.02),
            t + "embeddings.position_embedding.weight": det_tensor(seed, "t.pos", (c.max_position_embeddings, d), 0.02),
            t + "final_layer_norm.weight": det_tensor(seed, "t.final.w", (d,), 0.05, 1.0),
            t + "final_layer_norm.bias": det_tensor(seed, "t.final.b", (d,), 0.02),
            "text_projection.weight": det_tensor(seed, "t.proj", (c.projection_dim, d), 0.02),
        }
        for i in range(c.num_hidden_layers):
            p = t + f"encoder.layers.{i}."
            for nm in ("q_proj", "k_proj", "v_proj", "out_proj"):
                sd[p + f"self_attn.{nm}.weight"] = det_tensor(seed, p + nm + ".w", (d, d), 0.02)
                sd[p + f"self_attn.{nm}.bias"] = det_tensor(seed, p + nm + ".b", (d,), 0.02)
            sd[p + "layer_norm1.weight"] = det_tensor(seed, p + "ln1.w", (d,), 0.05, 1.0)
            sd[p + "layer_norm1.bias"] = det_tensor(seed, p + "ln1.b", (d,), 0.02)
            sd[p + "layer_norm2.weight"] = det_tensor(seed, p + "ln2.w", (d,), 0.05, 1.0)
            sd[p + "layer_norm2.bias"] = det_tensor(seed, p + "ln2.b", (d,), 0.02)
            sd[p + "mlp.fc1.weight"] = det_tensor(seed, p + "fc1.w", (c.intermediate_size, d), 0.02)
            sd[p + "mlp.fc1.bias"] = det_tensor(seed, p + "fc1.b", (c.intermediate_size,), 0.02)
            sd[p + "mlp.fc2.weight"] = det_tensor(seed, p + "fc2.w", (d, c.intermediate_size), 0.02)
            sd[p + "mlp.fc2.bias"] = det_tensor(seed, p + "fc2.b", (d,), 0.02)
        m.load_state_dict(sd, strict=True)
        return m

    @property
    def device(self):
        return self.text_projection.weight.device

    def check_ids(self, input_ids: Tensor) -> None:
        """The argument rules of the tower: [B, L] ids, L within the position table, and (whenever the ids are a
        host tensor) every id inside the vocabulary."""
        c = self.config
        if input_ids.dim() != 2:
            raise ValueError("CLIP text tower: input_ids must be [B, L]")
        L_ = input_ids.shape[1]
        if L_ < 1 or L_ > c.max_position_embeddings:
            raise ValueError(f"CLIP text tower: L = {L_} outside 1 ... {c.max_position_embeddings} (the position table)")
        if not input_ids.is_cuda and input_ids.numel() and (
                int(input_ids.min()) < 0 or int(input_ids.max()) >= c.vocab_size):
            raise ValueError(f"CLIP text tower: token ids outside the vocabulary [0, {c.vocab_size})")

    def get_text_features(self, input_ids: Tensor, attention_mask: Optional[Tensor] = None,
                          compute_dtype: torch.dtype = torch.bfloat16) -> Tensor:
        """Projected (un-normalised) text features [B, projection_dim] fp32. attention_mask is accepted and ignored:
        the tower is causal and pools the EOT row, which no padding position can reach. Not part of this build: the
        device schedule is left out, and there is no host fallback."""
        self.check_ids(input_ids)
        raise L.IcapError("CLIPTextTower.get_text_features: the device schedule of the CLIP text tower is not part "
                          "of this build (DESIGN.md, \"CLIP text tower\"); there is no host fallback")

    def embed(self, input_ids: Tensor, attention_mask: Optional[Tensor] = None,
              compute_dtype: torch.dtype = torch.bfloat16) -> Tensor:
        """L2-normalised features (src/embeddings/word_embeddings.py:75-78); see get_text_features."""
        return self.get_text_features(input_ids, attention_mask, compute_dtype)


# ------------------------------------------------------------ reference-shaped API (word_embeddings.py:11-171)


def load_clip_text_model(model_name: str = "openai/clip-vit-base-patch32", device: Optional[torch.device] = None,
                         checkpoint: Optional[str] = None) -> CLIPTextTower:
    """The text half of load_clip_model (src/embeddings/clip.py:10-35). Offline: weights come from `checkpoint` (HF
    safetensors / .bin state dict of CLIPModel, text keys used) when given, else a deterministic random init of the
    named architecture. No tokenizer is returned: no CLIP vocabulary exists offline, so the caller supplies any
    processor whose call returns `input_ids`."""
    device = device or torch.device("cuda")
    cfg = CLIPTextConfig.vit_l14() if "large-patch14" in model_name else CLIPTextConfig()
    if checkpoint is not None:
        model = CLIPTextTower(cfg)
        model.load_state_dict(_load_text_state(checkpoint), strict=False)
    else:
        model = CLIPTextTower.random_init(cfg)
    return model.to(device).eval()


def _load_text_state(path: str):
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file

        sd = load_file(path)
    else:
        sd = torch.load(path, map_location="cpu", weights_only=True)
    return {k: v for k, v in sd.items()
            if (k.startswith("text_model.") and not k.endswith("position_ids")) or k == "text_projection.weight"}


def load_image_embeddings_file_names(image_dir: str) -> List[str]:
    """word_embeddings.py:11-19: the filenames of an image-embedding .pt file."""
    return torch.load(image_dir, weights_only=True)["filenames"]


def load_captions_annotations(file_name: str) -> list:
    """word_embeddings.py:22-27: the `annotations` list of a COCO captions file."""
    with open(file_name, "r") as f:
        return json.load(f)["annotations"]


def get_image_id_from_filename(filename: str) -> int:
    """word_embeddings.py:30-36: 'COCO_train2014_000000123456.jpg' -> 123456."""
    return int(filename.split("_")[-1].split(".")[0])


def map_caption_id_to_caption(annotations_list):
    """word_embeddings.py:39-45: image id -> [{"caption_id", "caption"}] in annotation order."""
    image_to_captions = defaultdict(list)
    for ann in annotations_list:
        image_to_captions[ann["image_id"]].append({"caption_id": ann["id"], "caption": ann["caption"]})
    return image_to_captions


def _token_ids(clip_processor, captions, **kw) -> Tuple[Tensor, Optional[Tensor]]:
    """input_ids (and attention_mask, if any) of a duck-typed processor's output (mapping or attribute access)."""
    enc = clip_processor(text=captions, return_tensors="pt", **kw)
    get = enc.get if hasattr(enc, "get") else (lambda k, d=None: getattr(enc, k, d))
    return torch.as_tensor(get("input_ids"), dtype=torch.int64), get("attention_mask", None)


@torch.no_grad()
def extract_clip_embedding_from_caption(caption: str, clip_model, clip_processor,
                                        device: Optional[torch.device] = None) -> Tensor:
    """word_embeddings.py:48-82: one caption -> normalised (embedding_dim,) embedding (`clip_model.embed`)."""
    ids, mask = _token_ids(clip_processor, [caption], padding=True)
    return clip_model.embed(ids.to(device or clip_model.device), attention_mask=mask).squeeze(0)


@torch.no_grad()
def extract_caption_embeddings(image_embedding_file: str, annotations_file: str, output_path: str, clip_model,
                               clip_processor, batch_size: int = 256, normalize: bool = False,
                               device: Optional[torch.device] = None) -> int:
    """word_embeddings.py:85-171 as a function: the captions of every image of `image_embedding_file`, in filename
    order, tokenised per batch (`clip_processor(text=..., return_tensors="pt", padding=True, truncation=True)`) and
    embedded by `clip_model`; saved as the reference's list of {"filenames": name, "embeddings": [{"caption_id",
    "embedding": float32 ndarray [D]}]} in first-seen order — the file build_retrieval_store reads.
    normalize=False stores the un-normalised `get_text_features` output, as the reference's batch path does
    (:139-140) — unlike its single-caption function (:78), which normalises; normalize=True stores `embed`'s unit
    rows. Returns the number of captions embedded. (The reference's loop calls the `tqdm` module instead of
    `tqdm.tqdm`, :5,128, and cannot run as written; there is no progress bar here.)"""
    device = device or clip_model.device
    file_names = load_image_embeddings_file_names(image_embedding_file)
    image_to_captions = map_caption_id_to_caption(load_captions_annotations(annotations_file))
    all_captions_data = []
    for filename in file_names:
        for cap in image_to_captions.get(get_image_id_from_filename(filename), []):
            all_captions_data.append({"filename": filename, "caption_id": cap["caption_id"], "caption": cap["caption"]})
    print(f"Total captions to process: {len(all_captions_data)}")
    processed = {}
    fn = clip_model.embed if normalize else clip_model.get_text_features
    for i in range(0, len(all_captions_data), batch_size):
        batch = all_captions_data[i:i + batch_size]
        ids, mask = _token_ids(clip_processor, [item["caption"] for item in batch], padding=True, truncation=True)
        embeddings = fn(ids.to(device), attention_mask=mask).float().cpu().numpy()
        for j, item in enumerate(batch):
            processed.setdefault(item["filename"], []).append(
                {"caption_id": item["caption_id"], "embedding": embeddings[j].copy()})
    processed_data = [{"filenames": name, "embeddings": embs} for name, embs in processed.items()]
    torch.save(processed_data, output_path)
    print(f"Saved {len(all_captions_data)} caption embeddings of {len(processed_data)} images to {output_path}.")
    return len(all_captions_data)
