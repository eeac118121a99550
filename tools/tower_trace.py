"""Regenerates tests/golden/tower_traces.json: the launch trace of the four frozen encoder towers (CLIP vision, ViT,
DINOv3, CLIP text) at their real configurations, recorded on the CPU with tests/dryrun.py — nothing is launched and
nothing is computed. A case is one `features()` call of one core: every C-ABI call it makes, with every scalar
argument and struct field by value and every pointer replaced by the index of that address's first appearance in
the case (0 = NULL), so the aliasing structure and the leading dimensions are kept and the addresses are not. Which
arguments are pointers is read from the binding's own signatures (icap._lib.SIGNATURES, the structs' _fields_). The
file holds, per case, each call's name with 12 hex digits of SHA-256 over its canonical JSON, and one hash over
the whole case; tests/test_tower_trace_cpu.py compares a fresh recording with it call by call, so a change to a
tower's host schedule that moves, adds, drops or re-points a launch names the first call that differs. Needs no GPU
and no built library.

usage: python tools/tower_trace.py [output.json]"""

import ctypes as C
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gpt2-image-captioning_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from dryrun import dry_run  # noqa: E402
from icap import _lib  # noqa: E402
from icap import gpt2 as _gpt2  # noqa: E402
from icap.clip import CLIPVisionConfig, CLIPVisionTower, ClipCore  # noqa: E402
from icap.clip_text import CLIPTextConfig, CLIPTextTower, ClipTextCore  # noqa: E402
from icap.dino import DinoConfig, DINOv3ImageTower, DinoCore  # noqa: E402
from icap.vit import ViTConfig, ViTCore, ViTImageTower  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "tower_traces.json")

IMAGE_BATCH = 3
TEXT_SHAPES = ((6, 77), (3, 1), (300, 32))  # (B, L); the last one splits into two chunks (chunk_captions)
F32, BF16 = torch.float32, torch.bfloat16


class _DeviceIds(torch.Tensor):
    """Host ids that answer is_cuda like device ids: the text tower has no host path and checks for it, and a dry
    run has only host tensors."""
    is_cuda = property(lambda self: True)


def towers():
    """[(tower name, config, tower class, core class, [(variant, dtype, LayerNorm-fold switch)], [input shape])]"""
    clip_variants = [("fp32", F32, True), ("bf16_fold", BF16, True), ("bf16_nofold", BF16, False)]
    plain = [("fp32", F32, True), ("bf16", BF16, True)]
    px = [(IMAGE_BATCH, 3, 224, 224)]
    return [("clip_b32", CLIPVisionConfig(), CLIPVisionTower, ClipCore, clip_variants, px),
            ("clip_l14", CLIPVisionConfig.vit_l14(), CLIPVisionTower, ClipCore, clip_variants, px),
            ("vit_b16", ViTConfig(), ViTImageTower, ViTCore, plain, px),
            ("dinov3_l16", DinoConfig(), DINOv3ImageTower, DinoCore, plain, px),
            ("clip_text_b32", CLIPTextConfig(), CLIPTextTower, ClipTextCore, plain, TEXT_SHAPES),
            ("clip_text_l14", CLIPTextConfig.vit_l14(), CLIPTextTower, ClipTextCore, plain, TEXT_SHAPES)]


def traces():
    """Yields (case name, tower config, recorded calls of features(), out-of-bounds findings of those calls) for
    every case. The core is built first (its refresh converts the weights: not part of the trace)."""
    for tname, cfg, tower_cls, core_cls, variants, shapes in towers():
        with dry_run() as rec:
            tower = tower_cls(cfg)
            for vname, dtype, fold in variants:
                saved = _gpt2.TRAIN_LN_FOLD
                _gpt2.TRAIN_LN_FOLD = fold
                try:
                    core = core_cls(tower, dtype)
                finally:
                    _gpt2.TRAIN_LN_FOLD = saved
                for shape in shapes:
                    if len(shape) == 2:
                        case = f"{tname}/{vname}/B{shape[0]}_L{shape[1]}"
                        x = torch.ones(shape, dtype=torch.int64).as_subclass(_DeviceIds)
                    else:
                        case = f"{tname}/{vname}"
                        x = torch.zeros(shape)
                    n0, b0 = len(rec.calls), len(rec.bad)
                    core.features(x)
                    yield case, cfg, rec.calls[n0:], rec.bad[b0:]
                del core


def _canonical(calls):
    """The calls of one case as JSON-ready lists: [name, arg, ...], a struct argument as [[field, value], ...]."""
    seen = {}

    def ptr(v):
        v = v.value if hasattr(v, "value") else v
        return seen.setdefault(int(v), len(seen) + 1) if v else 0

    def struct(s):
        return [[f, ptr(getattr(s, f)) if t is _lib.vp else getattr(s, f)] for f, t in s._fields_]

    out = []
    for name, args in calls:
        types = _lib.SIGNATURES[name][1]
        assert len(types) == len(args), name
        row = [name]
        for t, v in zip(types, args):
            if t is _lib.vp:
                row.append(ptr(v))
            elif isinstance(getattr(t, "_type_", None), type) and issubclass(t._type_, C.Structure):  # POINTER(struct)
                row.append(struct(v._obj))
            else:
                row.append(v)
        out.append(row)
    return out


def digest(calls):
    """{"calls": ["<name> <12 hex>", ...], "hash": 16 hex over the whole case}"""
    whole = hashlib.sha256()
    lines = []
    for row in _canonical(calls):
        text = json.dumps(row, separators=(",", ":")).encode()
        whole.update(text + b"\n")
        lines.append(f"{row[0]} {hashlib.sha256(text).hexdigest()[:12]}")
    return {"calls": lines, "hash": whole.hexdigest()[:16]}


def record():
    """{case: digest} of every case, in order."""
    return {case: digest(calls) for case, _cfg, calls, _bad in traces()}


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    got = record()
    with open(path, "w") as f:
        json.dump(got, f, indent=0)
        f.write("\n")
    print(f"{path}: {len(got)} cases, {sum(len(d['calls']) for d in got.values())} calls, "
          f"{os.path.getsize(path)} bytes")
    for case, d in got.items():
        print(f"  {case}: {len(d['calls'])} calls, {d['hash']}")
