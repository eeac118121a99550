"""icap_layernorm_bwd (ln_bwd8_kernel, ln_bwd_kernel, ln_param_reduce) and icap_ln_param_reduce_batch against the
fp64 reference, cases and bounds of tests/ln_bwd_refs.py (its docstring derives the bounds and shows where the
constants come from; test_ln_bwd_refs_cpu.py checks all of it without a GPU). Every call writes into
sentinel-filled outputs with a NaN-filled workspace, NaN rows where nothing may be read and NaN padding columns
in the inputs; every test prints its worst ratio of error to bound before it asserts, asserts the layout and
that the inputs are bit-identical afterwards, and repeats the call for bitwise-equal results.

Worst error / bound measured on an MI355X when the file was added, K_DX = K_P = 16 (the bf16 dx figures sit just
under 1 because half an ulp of the one rounding is most of a bf16 bound; a 9-row sum of bf16 dy is exact, so
most bf16 dbeta are 0):
  kernel                                  dx             dx_drop   dgamma         dbeta
  ln_bwd8_kernel<bf16, true,  3/4/5/6>    0.995 .. 0.996 0.995     0.150 .. 0.156 0.031 (accumulate; else 0)
  ln_bwd8_kernel<bf16, false, 3/4/5/6>    0.986 .. 0.996 (3: 32777 rows)
  ln_bwd8_kernel<f32,  true,  3/4/5/6>    0.127 0.100 0.105 0.126   0.130   0.180 0.133 0.137 0.139   0.130 0.112 0.114 0.114
  ln_bwd8_kernel<f32,  false, 3/4/5/6>    0.130 0.100 0.099 0.126
  ln_bwd_kernel<bf16>                     0.995          0.968     0.148          0.0064
  ln_bwd_kernel<f32>                      0.131          0.108     0.163          0.128
  the three-item batched reduce: bitwise the per-call reduce; a repeated call: the same bits in every case.
Nothing was found: every kernel met every bound, layout and repeat check at every case."""

import pytest
import torch

import ln_bwd_refs as R
from icap import _lib as L
from icap import ops

pytestmark = pytest.mark.gpu

bf, f32 = torch.bfloat16, torch.float32
NAN = float("nan")


def bits(t):
    return t.view(torch.int16 if t.dtype == bf else torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a.cpu()), bits(b.cpu()))


def padded(values, ld, dev, fill, off=0):
    """values [rows, D] as a [rows, D] view with row stride ld, `off` elements into a 16-byte aligned flat buffer
    that holds `fill` everywhere else. Returns (view, flat buffer)."""
    rows, D = values.shape
    flat = torch.full((rows * ld + 8,), fill, dtype=values.dtype, device=dev)
    assert flat.data_ptr() % 16 == 0
    v = flat[off:off + rows * ld].view(rows, ld)[:, :D]
    v.copy_(values)
    return v, flat


class Call:
    """The device buffers of one case and one icap_layernorm_bwd call on them."""

    def __init__(self, case, dev, dx_drop=None, defer=False):
        t = case.inputs()
        self.case, self.t = case, t
        rows, D, dt = case.rows, case.D, case.dtype
        self.x, self.x_flat = padded(t["x"], case.ldx, dev, NAN, case.x_off)
        self.dy, self.dy_flat = padded(t["dy"], case.lddy, dev, NAN)
        self.dres, self.dres_flat = padded(t["dres"], case.lddres, dev, NAN) if case.dres else (None, None)
        self.small = {k: (None if t[k] is None else t[k].to(dev)) for k in ("gamma", "mean", "rstd", "rowmap")}
        self.rows_dev = None if case.rows_dev is None else torch.tensor([case.rows_dev], dtype=torch.int32, device=dev)
        self.dx = torch.full((rows, case.lddx), R.SENTINEL, dtype=dt, device=dev)
        want_drop = case.drop_p > 0 if dx_drop is None else dx_drop
        self.dxd = torch.full((rows, case.lddx), R.SENTINEL, dtype=dt, device=dev) if want_drop else None
        self.dg = t["dgamma0"].to(dev) if case.dgamma else None
        self.db = t["dbeta0"].to(dev) if case.dbeta else None
        self.ws = None
        if case.params:
            self.ws = torch.full((ops.layernorm_bwd_workspace(rows, D),), 0xFF, dtype=torch.uint8, device=dev)
            assert self.ws.numel() == R.launch(case)[0] * 2 * D * 4
        drop = ops.NO_DROP
        if want_drop:
            d, ctr = R.make_desc(case.drop_p, case.big)
            self.counter = None if ctr is None else torch.full((1,), ctr, dtype=torch.int64, device=dev)
            drop = ops.Dropout(d.p, d.seed, d.offset, self.counter)
        s = self.small
        ops.layernorm_bwd(self.x, s["gamma"], s["mean"], s["rstd"], self.dy, self.dx[:, :D],
                          dres=self.dres, dx_drop=None if self.dxd is None else self.dxd[:, :D], drop=drop,
                          dgamma=self.dg, dbeta=self.db, workspace=self.ws, rows=rows, dy_rowmap=s["rowmap"],
                          rows_dev=self.rows_dev, param_accumulate=case.accumulate, defer_params=defer)
        torch.cuda.synchronize()

    def inputs_intact(self):
        """x, dy, dres with their padding, gamma, the statistics and the row map hold the bits they were given."""
        c, t = self.case, self.t
        for view, flat, src, ld, off in ((self.x, self.x_flat, t["x"], c.ldx, c.x_off),
                                         (self.dy, self.dy_flat, t["dy"], c.lddy, 0),
                                         (self.dres, self.dres_flat, t["dres"], c.lddres, 0)):
            if flat is None:
                continue
            want = torch.full(flat.shape, NAN, dtype=flat.dtype)
            want[off:off + c.rows * ld].view(c.rows, ld)[:, :c.D] = src
            if not same_bits(flat, want):
                return False
        ok = same_bits(self.small["gamma"], t["gamma"]) and same_bits(self.small["mean"], t["mean"])
        ok = ok and same_bits(self.small["rstd"], t["rstd"])
        if t["rowmap"] is not None:
            ok = ok and torch.equal(self.small["rowmap"].cpu(), t["rowmap"])
        return ok

    def item(self):
        """This (deferred) call's entry of ops.ln_param_reduce_batch."""
        return (self.ws, self.case.rows, self.case.D, self.dg, self.db, self.case.accumulate)


def check(case, c):
    """Every assertion on one finished call; returns its ratios (dx, dx_drop, dgamma, dbeta)."""
    n, D = case.live, case.D
    dx = c.dx.cpu()
    r_dx = R.dx_ratio(case, dx)
    r_dg, r_db = R.param_ratios(case, c.dg, c.db)
    r_dxd = 0.0
    if c.dxd is not None:
        r_dxd = R.dx_drop_ratio(case, c.dxd)
    print(f"{case} -> {case.reaches}: error / bound dx {r_dx:.3g}, dx_drop {r_dxd:.3g}, dgamma {r_dg:.3g}, "
          f"dbeta {r_db:.3g}")
    assert R.untouched(case, dx), "dx: an element outside the live rows' D columns changed, or one inside did not"
    assert c.inputs_intact(), "an input changed"
    if c.dxd is not None:
        dxd = c.dxd.cpu()
        assert torch.equal(dxd[n:], torch.full_like(dxd[n:], R.SENTINEL))
        assert torch.equal(dxd[:, D:], torch.full_like(dxd[:, D:], R.SENTINEL))
        # the zero pattern is the mask's, exactly (a row whose dy the row map zeroes has dx == 0 without dres)
        assert torch.equal(dxd[:n, :D] == 0, ~case.keep()[:n] | (dx[:n, :D] == 0))
    assert r_dx <= 1.0 and r_dxd <= 1.0 and r_dg <= 1.0 and r_db <= 1.0
    return r_dx, r_dxd, r_dg, r_db


@pytest.mark.parametrize("case", R.CASES, ids=repr)
def test_layernorm_bwd(dev, case):
    c = Call(case, dev)
    check(case, c)
    if case.rows_dev == 0 and case.params:   # a dead call that overwrites stores exact zeros
        for g in (c.dg, c.db):
            assert g is None or torch.equal(g.cpu(), torch.zeros(case.D))
    # the sums run in a fixed order: a second call stores the same bits
    c2 = Call(case, dev)
    assert same_bits(c2.dx, c.dx)
    assert (c.dxd is None) or same_bits(c2.dxd, c.dxd)
    assert (c.dg is None or same_bits(c2.dg, c.dg)) and (c.db is None or same_bits(c2.db, c.db))
    if c.dxd is not None:   # dx does not depend on whether dx_drop is asked for
        c3 = Call(case, dev, dx_drop=False)
        assert same_bits(c3.dx, c.dx)
        assert (c.dg is None or same_bits(c3.dg, c.dg)) and (c.db is None or same_bits(c3.db, c.db))


def test_deferred_param_reduce_batch(dev):
    """Three deferred calls of unlike width and block count reduced by one icap_ln_param_reduce_batch: against
    fp64, and bitwise what each call's own reduce stores."""
    calls = [Call(case, dev, defer=True) for case in R.BATCH_CASES]
    for case, c in zip(R.BATCH_CASES, calls):   # deferred: the gradients still hold what they were given
        for got, init in ((c.dg, "dgamma0"), (c.db, "dbeta0")):
            assert got is None or same_bits(got, c.t[init])
    ops.ln_param_reduce_batch([c.item() for c in calls])
    torch.cuda.synchronize()
    for case, c in zip(R.BATCH_CASES, calls):
        check(case, c)
        own = Call(case, dev)
        assert same_bits(own.dx, c.dx)
        assert (c.dg is None or same_bits(own.dg, c.dg)) and (c.db is None or same_bits(own.db, c.db))
    # the same batch again from fresh calls: the same bits
    again = [Call(case, dev, defer=True) for case in R.BATCH_CASES]
    ops.ln_param_reduce_batch([c.item() for c in again])
    torch.cuda.synchronize()
    for c, a in zip(calls, again):
        assert (c.dg is None or same_bits(a.dg, c.dg)) and (c.db is None or same_bits(a.db, c.db))


def _as_strided(rows, D, ld, dtype, dev, fill):
    buf = torch.full((rows * ld + 8,), fill, dtype=dtype, device=dev)
    return buf.as_strided((rows, D), (ld, 1)), buf


@pytest.mark.parametrize("dtype", [bf, f32], ids=R.dt_name)
@pytest.mark.parametrize("rej", R.REJECTED, ids=repr)
def test_layernorm_bwd_rejects(dev, dtype, rej):
    """Refused on the host with an error: nothing is launched, every output still holds what it held."""
    rows, D = 9, rej.D
    x, _ = _as_strided(rows, D, rej.ldx, dtype, dev, 1.0)
    dy, _ = _as_strided(rows, D, rej.lddy, dtype, dev, 1.0)
    dres, _ = _as_strided(rows, D, rej.lddres, dtype, dev, 1.0)
    dx, dx_buf = _as_strided(rows, D, rej.lddx, dtype, dev, R.SENTINEL)
    dxd, dxd_buf = _as_strided(rows, D, rej.lddx, dtype, dev, R.SENTINEL)
    g = torch.ones(D, device=dev)
    stat = torch.ones(rows, device=dev)
    dg, db = torch.full((D,), R.SENTINEL, device=dev), torch.full((D,), R.SENTINEL, device=dev)
    ws = torch.full((ops.layernorm_bwd_workspace(rows, D),), 0xFF, dtype=torch.uint8, device=dev)
    drop = ops.Dropout(rej.drop_p, 1, 0) if rej.drop_p > 0 else ops.NO_DROP
    with pytest.raises(L.IcapError) as e:
        ops.layernorm_bwd(x, g, stat, stat, dy, dx, dres=dres, dx_drop=dxd if rej.drop_p > 0 else None, drop=drop,
                          dgamma=dg, dbeta=db, workspace=ws if rej.workspace else None, rows=rows)
    print(rej, "->", e.value)
    torch.cuda.synchronize()
    for t in (dx_buf, dxd_buf, dg, db):
        assert torch.equal(t, torch.full_like(t, R.SENTINEL))
    assert torch.equal(ws, torch.full_like(ws, 0xFF))
    if rej.why.startswith("ld"):
        assert "strides must be multiples of 4" in str(e.value)


@pytest.mark.parametrize("dtype", [bf, f32], ids=R.dt_name)
def test_layernorm_bwd_zero_rows(dev, dtype):
    """rows = 0 returns without a launch: dx, the gradients and the workspace keep what they held."""
    D = 768
    x = torch.ones((4, D), dtype=dtype, device=dev)
    dx = torch.full((4, D), R.SENTINEL, dtype=dtype, device=dev)
    g, stat = torch.ones(D, device=dev), torch.ones(4, device=dev)
    dg, db = torch.full((D,), R.SENTINEL, device=dev), torch.full((D,), R.SENTINEL, device=dev)
    ws = torch.full((ops.layernorm_bwd_workspace(4, D),), 0xFF, dtype=torch.uint8, device=dev)
    for acc in (False, True):
        ops.layernorm_bwd(x, g, stat, stat, x, dx, dres=x, dgamma=dg, dbeta=db, workspace=ws, rows=0,
                          param_accumulate=acc)
    torch.cuda.synchronize()
    for t in (dx, dg, db):
        assert torch.equal(t, torch.full_like(t, R.SENTINEL))
    assert torch.equal(ws, torch.full_like(ws, 0xFF))
