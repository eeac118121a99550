"""The JPEG test grid shared by test_jpeg_cpu.py and test_jpeg_gpu.py: files written by Pillow into memory from a fixed
seed (no committed image), and Pillow's own decode of each as the reference."""

import io

import numpy as np
from PIL import Image

SIZES = [(1, 1), (8, 8), (13, 17), (16, 16), (3, 5), (5, 3), (33, 47), (48, 64), (2, 40), (40, 2), (17, 4), (9, 6)]
CONTENTS = ["noise", "gradient", "flat"]
# name -> (grayscale, Image.save keywords)
ENCODINGS = {
    "q30-420": (False, dict(quality=30, subsampling="4:2:0")),
    "q75-420-opt": (False, dict(quality=75, subsampling="4:2:0", optimize=True)),
    "q95-422": (False, dict(quality=95, subsampling="4:2:2")),
    "q100-444": (False, dict(quality=100, subsampling="4:4:4")),
    "q90-420-rst-blocks1": (False, dict(quality=90, subsampling="4:2:0", restart_marker_blocks=1)),
    "q85-422-rst-rows1": (False, dict(quality=85, subsampling="4:2:2", restart_marker_rows=1)),
    "q5-420": (False, dict(quality=5, subsampling="4:2:0")),
    "gray-q80": (True, dict(quality=80)),
}


def content(kind: str, h: int, w: int, seed: int = 0) -> np.ndarray:
    """RGB uint8 [h, w, 3]: uniform noise; per-channel gradients; a flat 200 field with isolated zero pixels every
    5 x 7 and a saturated half."""
    if kind == "noise":
        return np.random.default_rng(1234 + seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "gradient":
        y, x = np.mgrid[0:h, 0:w]
        return np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1),
                         ((x + y) * 255) // max(h + w - 2, 1)], -1).astype(np.uint8)
    a = np.full((h, w, 3), 200, dtype=np.uint8)
    a[::5, ::7] = 0
    a[:, w // 2:] = 255
    a[h // 2::5, w // 2::7] = 0
    return a


def encode(arr: np.ndarray, enc: str) -> bytes:
    gray, kw = ENCODINGS[enc]
    im = Image.fromarray(arr)
    buf = io.BytesIO()
    (im.convert("L") if gray else im).save(buf, format="JPEG", **kw)
    return buf.getvalue()


def reference(data: bytes) -> np.ndarray:
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


_GRID = None


def grid():
    """[(id, file bytes, Pillow's RGB uint8 [H, W, 3])] for every size x content x encoding: 288 files, built once."""
    global _GRID
    if _GRID is None:
        _GRID = []
        for h, w in SIZES:
            for kind in CONTENTS:
                for enc in ENCODINGS:
                    data = encode(content(kind, h, w), enc)
                    _GRID.append((f"{h}x{w}-{kind}-{enc}", data, reference(data)))
    return _GRID


def big_file(h: int, w: int, seed: int = 7, **kw) -> bytes:
    """Gradient plus noise, q90 4:2:0 unless kw says otherwise."""
    g = content("gradient", h, w).astype(np.int32)
    nz = np.random.default_rng(seed).integers(-24, 25, (h, w, 3))
    buf = io.BytesIO()
    opts = dict(quality=90, subsampling="4:2:0")
    opts.update(kw)
    Image.fromarray(np.clip(g + nz, 0, 255).astype(np.uint8)).save(buf, format="JPEG", **opts)
    return buf.getvalue()
