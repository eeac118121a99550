"""icap_gemm_group on 128 x 256 tiles (round 10: gemm_group256_kernel, csrc/gemm_tile_roles_kout.hip): a group whose tiles
then fit one round of one block per compute unit runs the K-outer split-role body with 8 MFMA waves of 64 x 64 on a
ring of 3 stages of 64 k-rows x (128 + 256) columns; a product with one output column (a bias gradient against a ones
column) runs with its operands exchanged and stores its tile transposed. Per output element the MFMA chain is the
128 x 128 body's, so every comparison here is bitwise (torch.equal on the fp32 outputs): against the same products run
one by one through ops.gemm(trans_ab=True, split_k=1, roles=1) — the unsplit K-outer split-role kernel in natural K
order, what include/icap.h documents the group equal to (the automatic plan rotates the k-step order of its tile
kernels per tile, another fp32 summation order: the group was never bitwise that) — and against the group with
ICAP_GROUP128=1, which forces the 128 x 128 body (looked up at every grouped call)."""

import os

import pytest
import torch

from icap import CaptionTrainer, ops
from gemm_helpers import _assert_same, rnd

pytestmark = pytest.mark.gpu

SHAPES = [  # (output rows, output columns, K)
    (128, 256, 64),    # one tile, one k-step
    (128, 256, 192),   # the ring's depth
    (128, 256, 256),   # one past it
    (128, 256, 200),   # a K tail
    (136, 264, 200),   # one row chunk and one column chunk past a tile
    (768, 768, 320),
    (256, 3072, 128),
]


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _tiles256(items):
    """Tiles of a group on the 128 x 256 body (csrc/gemm_plan.cpp gemm_group_plan)."""
    n = 0
    for it in items:
        M, N = it[3], it[4]
        n += -(-M // 256) if N <= 4 else -(-M // 128) * -(-N // 256)
    return n


def _operands(dev, M, N, K, seed):
    dY = rnd((K, M + (-M) % 8), dev, scale=0.2, seed=seed)
    X = rnd((K, N + (-N) % 8), dev, seed=seed + 1)
    G = rnd((M, N), dev, torch.float32, 1.0, seed=seed + 2)
    return dY, X, G


class _force128:
    def __enter__(self):
        os.environ["ICAP_GROUP128"] = "1"

    def __exit__(self, *exc):
        os.environ.pop("ICAP_GROUP128", None)


def _check_group(dev, specs, expect_big=True):
    """specs: (A, B, C0, M, N, K, beta). Runs the group (new body), the group under the override and the products one by
    one; asserts all three bitwise equal. Returns the group's outputs."""
    new = [(A, B, C0.clone(), M, N, K, beta) for A, B, C0, M, N, K, beta in specs]
    old = [(A, B, C0.clone(), M, N, K, beta) for A, B, C0, M, N, K, beta in specs]
    one = [(A, B, C0.clone(), M, N, K, beta) for A, B, C0, M, N, K, beta in specs]
    assert (_tiles256(specs) <= _cus(dev)) == expect_big
    ops.gemm_group(new)
    with _force128():
        ops.gemm_group(old)
    for A, B, C, M, N, K, beta in one:
        ops.gemm(A, B, C, beta=beta, M=M, N=N, K=K, trans_ab=True, split_k=1, roles=1)
    torch.cuda.synchronize()
    for i, (a, b, c) in enumerate(zip(new, old, one)):
        _assert_same(f"product {i}: 128 x 256 body vs one by one", a[2], c[2])
        _assert_same(f"product {i}: 128 x 256 body vs 128 x 128 body", a[2], b[2])
    return [it[2] for it in new]


@pytest.mark.parametrize("M,N,K", SHAPES)
@pytest.mark.parametrize("beta", [0.0, 1.0])
def test_group256_one_product(dev, M, N, K, beta):
    dY, X, G = _operands(dev, M, N, K, 1)
    C, = _check_group(dev, [(dY, X, G, M, N, K, beta)])
    ref = dY[:, :M].double().t() @ X[:, :N].double() + beta * G.double()
    bound = dY[:, :M].double().abs().t() @ X[:, :N].double().abs() + beta * G.double().abs()
    assert ((C.double() - ref).abs() / bound).max().item() < 1e-5


def test_group256_four_products_two_bias_gradients(dev):
    """Four products of different shapes, bias gradients (ones column, N = 1, C viewed [M, 1]) on two of them: the bias
    outputs bitwise too, and equal to the fp64 column sums to fp32 accumulation order."""
    K = 328
    ones = torch.ones((K, 8), device=dev, dtype=torch.bfloat16)
    specs = []
    for i, (M, N, beta) in enumerate([(768, 768, 1.0), (136, 264, 0.0), (520, 200, 1.0), (256, 1032, 1.0)]):
        specs.append(_operands(dev, M, N, K, 10 + 3 * i) + (M, N, K, beta))
    db0 = rnd((768, 1), dev, torch.float32, 1.0, seed=40)
    db2 = rnd((520, 1), dev, torch.float32, 1.0, seed=41)
    specs.append((specs[0][0], ones, db0, 768, 1, K, 1.0))
    specs.append((specs[2][0], ones, db2, 520, 1, K, 0.0))
    out = _check_group(dev, specs)
    for got, dY, M, base in ((out[4], specs[0][0], 768, db0), (out[5], specs[2][0], 520, None)):
        ref = dY[:, :M].double().sum(0) + (base.double().view(-1) if base is not None else 0.0)
        err = ((got.double().view(-1) - ref).abs() / (dY[:, :M].double().abs().sum(0) + 1.0)).max().item()
        assert err < 1e-5, err


def test_group256_more_tiles_than_cus_falls_back(dev):
    """1024 x 8448 is 8 x 33 = 264 tiles of 128 x 256: more than one round on 256 compute units, so the launcher keeps
    the 128 x 128 body. Equal either way."""
    M, N, K = 1024, 8448, 64
    dY, X, G = _operands(dev, M, N, K, 50)
    _check_group(dev, [(dY, X, G, M, N, K, 1.0)], expect_big=_cus(dev) >= 264)


def test_group256_exactly_one_round(dev):
    """As many 128 x 256 tiles as the device has compute units (one product of cus row tiles short of one, plus one
    more product of a single tile)."""
    cus = _cus(dev)
    K = 64
    a = _operands(dev, 128 * (cus - 1), 256, K, 60) + (128 * (cus - 1), 256, K, 1.0)
    b = _operands(dev, 128, 256, K, 63) + (128, 256, K, 0.0)
    assert _tiles256([a, b]) == cus
    _check_group(dev, [a, b])


def test_group256_writes_nothing_outside_its_outputs(dev):
    """C and the bias gradient with one spare row and one spare column, filled with sentinels."""
    M, N, K = 136, 264, 200
    dY, X, _ = _operands(dev, M, N, K, 70)
    ones = torch.ones((K, 8), device=dev, dtype=torch.bfloat16)
    S = -12345.5
    Cb = torch.full((M + 1, N + 1), S, device=dev)
    db = torch.full((M + 1, 2), S, device=dev)
    ops.gemm_group([(dY, X, Cb[:M, :N], M, N, K, 0.0), (dY, ones, db[:M, :1], M, 1, K, 0.0)])
    torch.cuda.synchronize()
    assert (Cb[M] == S).all() and (Cb[:, N] == S).all() and (db[M] == S).all() and (db[:, 1] == S).all()
    Cr = torch.empty((M, N), device=dev)
    dbr = torch.empty((M, 1), device=dev)
    ops.gemm(dY, X, Cr, beta=0.0, M=M, N=N, K=K, trans_ab=True, split_k=1, roles=1)
    ops.gemm(dY, ones, dbr, beta=0.0, M=M, N=1, K=K, trans_ab=True, split_k=1, roles=1)
    torch.cuda.synchronize()
    _assert_same("C", Cb[:M, :N].contiguous(), Cr)
    _assert_same("db", db[:M, :1].contiguous(), dbr)


def test_group256_repeatable(dev):
    M, N, K = 768, 768, 320
    dY, X, G = _operands(dev, M, N, K, 80)
    ones = torch.ones((K, 8), device=dev, dtype=torch.bfloat16)
    outs = []
    for _ in range(20):
        C, db = G.clone(), G[:, :1].clone()
        ops.gemm_group([(dY, X, C, M, N, K, 1.0), (dY, ones, db, M, 1, K, 1.0)])
        outs.append((C, db))
    torch.cuda.synchronize()
    for i, (C, db) in enumerate(outs[1:]):
        _assert_same(f"launch {i + 1}", C, outs[0][0])
        _assert_same(f"launch {i + 1} db", db, outs[0][1])


def test_group256_trainer_step_graph_equals_override(dev):
    """One graph-replayed CaptionTrainer step (tiny config, bf16, mapper_dw="fused") with the 128 x 256 body against
    the same step captured under the override: flat_grad bitwise equal."""
    from test_group_dw_gpu import _batch
    from test_model_gpu import TINY_G, TINY_M, build

    grads = []
    for force in (False, True):
        if force:
            os.environ["ICAP_GROUP128"] = "1"
        try:
            model = build(TINY_G, TINY_M, torch.bfloat16, dev)
            t = CaptionTrainer(model, 6, 14, lr=1e-3, num_training_steps=8, dropout=True, seed=3, mapper_dw="fused")
            t.load_batch(*_batch(1, dev))
            t.micro_step(use_graph=True)
            torch.cuda.synchronize()
            grads.append(t.flat.flat_grad.clone())
        finally:
            os.environ.pop("ICAP_GROUP128", None)
    assert torch.isfinite(grads[0]).all() and float(grads[0].abs().max()) > 0.0
    assert torch.equal(grads[0], grads[1]), f"{int((grads[0] != grads[1]).sum())} gradient entries differ"
