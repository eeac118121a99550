"""The whole train step with dropout on against the fp64 oracle drawing the device's own masks
(dropout_refs.MaskedOracle): the tiny captioner of test_model_gpu.py on test_pack_gpu.ragged_batch(7, 12), trainer
seed 5, lr 1e-3, two steps (the dropout counter advances between them; the second step is the graph replay under
use_graph). The reference is mapper_forward + caption_forward in fp64 under the hook, torch.autograd.grad over the
mapper, clip_and_adamw between the steps.

How far a wrong mask is from the bounds, measured with the reference alone on the CPU on this batch: drawing the 15
sites' masks with another counter value or seed moves every mapper tensor's gradient by at least 0.54 in relative L2
(test_dropout_refs_cpu.py holds > 0.1), the reference evaluated in fp32 is off by at most 5.7e-7 and in bf16 by at
most 0.053. The bounds: 1e-3 for fp32 (about 1700x that fp32 floor, 500x below a wrong mask) and 0.10 for bf16 (about
2x the CPU bf16 evaluation, 5x below a wrong mask).

Measured on MI355X (per-tensor relative L2 of the first step's mapper gradients, max over tensors; loss |rel d| max
over the two steps):
  fp32 padded, eager and graph: gradient 4.66e-07 (linear.weight), loss 1.56e-07
  fp32 packed, eager and graph: gradient 4.97e-07 (linear.weight), loss 7.78e-08
  bf16 packed graph:            gradient 0.0423 (transformer.layers.0.linear1.weight), loss |d| 3.2e-04 (5.3e-05 rel)
"""

import pytest
import torch

import dropout_refs as R
from icap import CaptionTrainer
from oracle import icap_oracle as O
from test_bf16w_gpu import TRAIN_LOSS_D
from test_model_gpu import TINY_G, TINY_M, build
from test_pack_gpu import pack_ref, ragged_batch

pytestmark = pytest.mark.gpu

B, LC, SEED, LR, STEPS, TOTAL = 7, 12, 5, 1e-3, 2, 4


def run_steps(dev, dtype, pack, graph):
    """Two trainer steps and the masked oracle's: (device losses, reference losses, {tensor: relative L2 of the first
    step's gradient})."""
    ids, mask, labels, emb = ragged_batch(B, LC, TINY_G.vocab_size, TINY_G.eos, TINY_M.embed_dim, seed=9)
    model = build(TINY_G, TINY_M, dtype, dev)
    t = CaptionTrainer(model, B, LC, lr=LR, num_training_steps=TOTAL, dropout=True, seed=SEED, pack_rows=pack)
    assert t.gws.pack == pack
    t.load_batch(ids, mask, labels, emb.to(dev))
    grows = None
    if pack:  # position (b, t) of the [B, S, D] sites is device row seq_off[b] + t; attention keeps (b, h, q, k)
        seq_off, seq_len = pack_ref(B, t.P, LC, mask, labels)[:2]
        grows = R.packed_rows(seq_off, seq_len, t.gws.S)
    msd = {k: v.double().requires_grad_(True) for k, v in O.mapper_state_dict(TINY_M, 0).items()}
    gsd = {k: v.double() for k, v in O.gpt2_state_dict(TINY_G, 0).items()}
    st = O.AdamWState()
    names = [k for k, _ in model.mapping_network.named_parameters()]
    assert set(names) == set(msd)
    dev_losses, ref_losses, grad_rel = [], [], {}
    for step in range(STEPS):
        t.micro_step(use_graph=graph)
        dev_losses.append(t.last_loss.item())
        assert int(t.counter) == step + 1  # one increment per step, before its first mask is drawn
        with R.MaskedOracle(t, TINY_M.num_layers, TINY_G.n_layer, grows):
            prefix = O.mapper_forward(msd, TINY_M, emb.double(), True, 0.1)
            loss, _ = O.caption_forward(gsd, TINY_G, prefix, ids, mask, labels, True, 0.1)
        grads = dict(zip(msd, torch.autograd.grad(loss, list(msd.values()))))
        ref_losses.append(float(loss.detach()))
        if step == 0:
            for k, prm in model.mapping_network.named_parameters():
                u = t.flat.grad(prm).detach().double().cpu().reshape(-1)
                r = grads[k].reshape(-1)
                grad_rel[k] = float((u - r).norm() / r.norm())
        with torch.no_grad():
            O.clip_and_adamw({k: v.data for k, v in msd.items()}, grads, st, LR, 0, TOTAL)
    return dev_losses, ref_losses, grad_rel


def report(tag, dev_losses, ref_losses, grad_rel):
    kmax = max(grad_rel, key=grad_rel.get)
    dl = [abs(a - b) / abs(b) for a, b in zip(dev_losses, ref_losses)]
    print(f"{tag}: losses {dev_losses} vs masked oracle {ref_losses} (rel |d| {max(dl):.3g}); first-step gradient "
          f"relative L2 max {grad_rel[kmax]:.3g} ({kmax})")
    return dl, grad_rel[kmax], kmax


@pytest.mark.parametrize("pack,graph", [(False, False), (False, True), (True, False), (True, True)])
def test_fp32_step_matches_masked_oracle(dev, pack, graph):
    """fp32: losses within 1e-5 relative (the bound of test_model_gpu.py's dropout-free steps), every mapper tensor's
    first-step gradient within 1e-3 relative L2."""
    dl, gmax, kmax = report(f"fp32 pack={pack} graph={graph}", *run_steps(dev, torch.float32, pack, graph))
    assert max(dl) < 1e-5, dl
    assert gmax <= 1e-3, (kmax, gmax)


def test_bf16_packed_graph_step_matches_masked_oracle(dev):
    """The benchmarked form (bf16, packed rows, graph replay): losses within TRAIN_LOSS_D, every mapper tensor's
    first-step gradient within 0.10 relative L2."""
    dev_losses, ref_losses, grad_rel = run_steps(dev, torch.bfloat16, True, True)
    _, gmax, kmax = report("bf16 packed graph", dev_losses, ref_losses, grad_rel)
    assert max(abs(a - b) for a, b in zip(dev_losses, ref_losses)) < TRAIN_LOSS_D
    assert gmax <= 0.10, (kmax, gmax)
