"""Trainer level: the step whose optimizer kernel writes the mapper's transposed weight copies itself
(engine.ADAM_TRANSPOSE, icap_adamw_args.items) against the same trainer with the transpose launch after the update.
Three steps (one eager, two replays of the captured graph), bf16, mapper_dw="fused": everything the step leaves
behind is compared byte for byte."""

import pytest
import torch

from icap import CaptionTrainer, engine
from test_model_gpu import TINY_G, TINY_M, build, inputs, load

pytestmark = pytest.mark.gpu


def _steps(dev, fused):
    saved = engine.ADAM_TRANSPOSE
    engine.ADAM_TRANSPOSE = fused
    try:
        ids, mask, labels, emb = inputs(load("tiny"), dev)
        model = build(TINY_G, TINY_M, torch.bfloat16, dev)
        t = CaptionTrainer(model, ids.shape[0], ids.shape[1], lr=1e-3, num_training_steps=6, dropout=True, seed=5,
                           mapper_dw="fused")
        assert (t._adam_items() is not None) and len(t._adam_items()) == 4 * t.mcore.nl
        t.load_batch(ids, mask, labels, emb)
        for _ in range(3):
            t.micro_step(use_graph=True)
        torch.cuda.synchronize()
        out = {"flat": t.flat.flat, "flat_c": t.flat.flat_c, "grad": t.flat.flat_grad, "m": t.flat.exp_avg,
               "v": t.flat.exp_avg_sq, "loss_sum": t.loss_sum, "state": t.adam_state}
        for i, (_, wt) in enumerate(t.mcore.transpose_pairs()):
            out[f"wt{i}"] = wt
        return {k: v.detach().clone() for k, v in out.items()}, t
    finally:
        engine.ADAM_TRANSPOSE = saved


def test_trainer_adam_transposes_bitwise(dev):
    new, t = _steps(dev, True)
    old, _ = _steps(dev, False)
    assert set(new) == set(old) and len([k for k in new if k.startswith("wt")]) == 4 * TINY_M.num_layers
    for k in old:
        assert torch.equal(new[k].view(torch.uint8), old[k].view(torch.uint8)), k
    # and the copies are the transposes of the weights the next forward reads
    for w, wt in t.mcore.transpose_pairs():
        assert torch.equal(wt, w.t())
    assert int(new["state"].view(torch.int64)[0].item()) == 3
