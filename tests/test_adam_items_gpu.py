"""icap_adamw_step with matrix items (icap_adamw_args.items): the update kernel writes the transposed bf16 copies of
those matrices itself. Everything it stores is compared byte for byte with the call without items followed by
icap_transpose_batch of its bf16_out."""

import pytest
import torch

from icap import ops

pytestmark = pytest.mark.gpu

HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, max_norm=1.0, num_warmup_steps=1,
          num_training_steps=10)


def layout(shapes, tail):
    """FlatParams' layout: every tensor starts on a 16-element boundary; `tail` loose elements end the buffer."""
    offs, o = [], 0
    for sh in shapes:
        offs.append(o)
        n = 1
        for d in sh:
            n *= d
        o = (o + n + 15) // 16 * 16
    return offs, o + tail


def gaps(shapes, offs, n):
    """Element ranges no tensor owns (alignment gaps)."""
    out = []
    for i, (sh, off) in enumerate(zip(shapes, offs)):
        cnt = 1
        for d in sh:
            cnt *= d
        nxt = offs[i + 1] if i + 1 < len(offs) else (n // 16 * 16)
        if off + cnt < nxt:
            out.append((off + cnt, nxt))
    return out


def run(dev, shapes, tail, steps=2, seed=0):
    """Both forms over the same inputs: {name: tensor} of the old call (+ transpose_batch) and of the call with
    items; bf16_out and the transposed copies start from a fill pattern, so untouched words show."""
    offs, n = layout(shapes, tail)
    mats = [(off, sh) for off, sh in zip(offs, shapes) if len(sh) == 2]
    g = torch.Generator(device="cpu").manual_seed(seed)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * 0.1 for _ in range(steps)]
    res = {}
    for mode in ("old", "items"):
        p = p0.to(dev)
        m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        out16 = torch.full((n,), 3.0, dtype=torch.bfloat16, device=dev)
        for lo, hi in gaps(shapes, offs, n):  # a distinct pattern in the gaps of every buffer
            p[lo:hi] = 11.0
            out16[lo:hi] = 13.0
        state = torch.zeros(16, dtype=torch.float32, device=dev)
        ws = torch.empty(ops.adamw_workspace(n), dtype=torch.uint8, device=dev)
        dsts = [torch.full((sh[1], sh[0]), 5.0, dtype=torch.bfloat16, device=dev) for _, sh in mats]
        for gr in grads:
            gd = gr.to(dev)
            if mode == "old":
                ops.adamw_step(p, gd, m, v, state, ws, bf16_out=out16, **HP)
                ops.transpose_batch([(out16[off:off + sh[0] * sh[1]].view(sh), d) for (off, sh), d in zip(mats, dsts)])
            else:
                ops.adamw_step(p, gd, m, v, state, ws, bf16_out=out16,
                               items=[(off, sh[0], sh[1], d) for (off, sh), d in zip(mats, dsts)], **HP)
        torch.cuda.synchronize()
        res[mode] = dict(p=p, m=m, v=v, out16=out16, state=state, **{f"t{i}": d for i, d in enumerate(dsts)})
    return res, offs, n


def same_bytes(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def test_adam_items_mixed_layout(dev):
    """A small vector, a one-tile matrix, a vector, a matrix whose 264 columns leave a partial column tile, a
    72-row matrix the tiles cannot take (falls back to the transpose launch inside the call), a 3-column-tile
    matrix and an n % 4 == 3 tail; two steps, so m and v are non-zero on entry to the second."""
    shapes = [(5,), (64, 8), (768,), (192, 264), (72, 24), (128, 768)]
    res, offs, n = run(dev, shapes, tail=3)
    assert n % 4 == 3
    old, new = res["old"], res["items"]
    for k in old:
        assert same_bytes(old[k], new[k]), k
    # the transposed copies are the transposes of the final bf16 mirror, fallback item included
    mats = [(off, sh) for off, sh in zip(offs, shapes) if len(sh) == 2]
    for i, (off, sh) in enumerate(mats):
        assert torch.equal(new[f"t{i}"], new["out16"][off:off + sh[0] * sh[1]].view(sh).t()), sh
    # (the words of the alignment gaps belong to the flat loop in both forms: the byte comparison above covers them,
    # each gap starting from its own pattern; test_adam_items_gap_words has the real-use case, where they stay zero)
    assert int(new["state"].view(torch.int64)[0].item()) == 2


def test_adam_items_real_shape(dev):
    """One 768 x 3072 matrix (144 tiles over many blocks) between two vectors."""
    shapes = [(768,), (768, 3072), (3072,)]
    res, offs, n = run(dev, shapes, tail=0, seed=1)
    old, new = res["old"], res["items"]
    for k in old:
        assert same_bytes(old[k], new[k]), k
    assert torch.equal(new["t0"], new["out16"][offs[1]:offs[1] + 768 * 3072].view(768, 3072).t())


def test_adam_items_gap_words(dev):
    """The alignment gaps hold zero parameters, gradients and moments in real use: both forms leave them zero, and
    every word of the transposed copies outside [cols, rows] (ldd > rows) keeps its fill."""
    shapes = [(5,), (64, 24), (7,)]
    offs, n = layout(shapes, 0)
    p = torch.zeros(n, device=dev)
    p[:5], p[offs[1]:offs[1] + 64 * 24], p[offs[2]:offs[2] + 7] = 1.0, 2.0, 3.0
    g = torch.zeros(n, device=dev)
    g[offs[1]:offs[1] + 64 * 24] = 0.5
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    out16 = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    wide = torch.full((24, 72), 5.0, dtype=torch.bfloat16, device=dev)  # ldd = 72 > rows = 64
    state = torch.zeros(16, dtype=torch.float32, device=dev)
    ws = torch.empty(ops.adamw_workspace(n), dtype=torch.uint8, device=dev)
    ops.adamw_step(p, g, m, v, state, ws, bf16_out=out16, items=[(offs[1], 64, 24, wide[:, :64])], **HP)
    torch.cuda.synchronize()
    for lo, hi in gaps(shapes, offs, n):
        for t in (p, m, v, out16):
            assert torch.all(t[lo:hi] == 0)
    assert torch.all(wide[:, 64:] == 5.0)
    assert torch.equal(wide[:, :64], out16[offs[1]:offs[1] + 64 * 24].view(64, 24).t())
