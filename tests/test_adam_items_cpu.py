"""No GPU: the optimizer call's matrix items (icap_adamw_args.items) — argument checks that run before any launch,
and the items the trainer hands over (recorded with tests/dryrun.py)."""

import ctypes as C

import pytest
import torch

import icap.weights
from dryrun import dry_run
from icap import CaptionTrainer, _lib, engine
from test_dryrun_bounds import batch, tiny_model


def _args(n, items, bf16_out=1 << 20):
    a = _lib.AdamWArgs()
    a.n = n
    a.params = a.grads = a.exp_avg = a.exp_avg_sq = 1 << 20  # never dereferenced: the checks are host-only
    a.state = 1 << 20
    a.bf16_out = bf16_out
    arr = (_lib.AdamWItem * len(items))()
    for it, (off, rows, cols, ldd) in zip(arr, items):
        it.offset, it.rows, it.cols, it.dst, it.ldd = off, rows, cols, 1 << 21, ldd
    a.n_items, a.items = len(items), C.cast(arr, C.c_void_p)
    return a, arr


@pytest.mark.parametrize("items,bf16_out,msg", [
    ([(0, 64, 8, 64), (256, 64, 8, 64)], 1 << 20, "items overlap"),            # second starts inside the first
    ([(1024, 64, 8, 64)], 1 << 20, "outside the flat buffer"),                 # 1024 + 512 > n
    ([(0, 64, 8, 56)], 1 << 20, "ldd < rows"),
    ([(0, 64, 8, 64)], None, "items need an item array and bf16_out"),
])
def test_item_checks_run_before_any_launch(items, bf16_out, msg):
    a, arr = _args(1200, items, bf16_out)
    with pytest.raises(_lib.IcapError, match=msg):
        _lib.call("icap_adamw_step", C.byref(a), 1 << 22, None)


def _optimizer_calls(dtype):
    with dry_run() as rec:
        icap.weights.ops.call = rec
        t = CaptionTrainer(tiny_model(dtype=dtype), 3, 12, num_training_steps=3)
        t.load_batch(*batch(3, 12))
        n0 = len(rec.calls)
        t._optimizer()
        names = [c[0] for c in rec.calls[n0:]]
        items = t._adam_items()
        return t, names, items


def test_trainer_hands_every_mapper_pair_to_the_optimizer():
    """bf16: 4 items per mapper layer at the weights' flat offsets, each [out, in] with its [in, out] copy, and no
    transpose launch after the update; the module constant restores it."""
    t, names, items = _optimizer_calls(torch.bfloat16)
    assert "icap_adamw_step" in names and "icap_transpose_batch" not in names and "icap_transpose" not in names
    pairs = t.mcore.transpose_pairs()
    assert len(items) == len(pairs) == 4 * t.mcore.nl
    offs = {id(p): o for p, o in zip(t.flat.params, t.flat.offsets)}
    lay = t.model.mapping_network.transformer.layers
    want = [offs[id(p)] for l in lay for p in (l.self_attn.in_proj_weight, l.self_attn.out_proj.weight,
                                               l.linear1.weight, l.linear2.weight)]
    assert [it[0] for it in items] == want
    for (off, rows, cols, dst), (w, wt) in zip(items, pairs):
        assert (rows, cols) == tuple(w.shape) and dst is wt and tuple(wt.shape) == (cols, rows)
        assert off % 16 == 0 and off + rows * cols <= t.flat.n
    ends = sorted((it[0], it[0] + it[1] * it[2]) for it in items)
    assert all(a[1] <= b[0] for a, b in zip(ends, ends[1:]))
    engine.ADAM_TRANSPOSE = False
    try:
        _, names, _ = _optimizer_calls(torch.bfloat16)
    finally:
        engine.ADAM_TRANSPOSE = True
    assert "icap_transpose_batch" in names


def test_fp32_parity_mode_keeps_its_transposes():
    t, names, items = _optimizer_calls(torch.float32)
    assert items is None and names.count("icap_transpose") == 4 * t.mcore.nl
