"""The GEMM epilogue of every kernel family per element against the fp64 references of tests/gemm_epi_refs.py: each
case launches the kernel instantiation it names (recorded, not assumed), C and aux are checked element by element
against the case's bounds (no max-norm, no exclusions, no retries), and everything a launch must not touch — padding
columns of the padded C / aux buffers, rows at or past the device row count, the read-only operands — must survive
bitwise. One test per family: a handful of small launches; the fp64 products are computed once per input set
(gemm_epi_refs.inputs is cached)."""

import pytest
import torch

import gemm_epi_refs as R
from gemm_epi_refs import CASES, SENTINEL, bf
from gemm_helpers import _run
from icap import ops

pytestmark = pytest.mark.gpu

FAMILY_NAMES = sorted({c.family for c in CASES})


def _padded(t, ld, off, dev, rows=None):
    """(buffer, view): t (CPU, [rows, N]) as the view buf[:, off:off + N] of a sentinel-filled [rows, ld] device
    buffer; t = (rows, N, dtype): an output, all sentinel."""
    if isinstance(t, tuple):
        rows, N, dt = t
        t = None
    else:
        (rows, N), dt = t.shape, t.dtype
    buf = torch.full((rows, ld), SENTINEL, dtype=dt, device=dev)
    view = buf[:, off:off + N]
    if t is not None:
        view.copy_(t)
    return buf, view


def _run_case(c, dev):
    x = c.inputs()
    M, N, K, lay = c.M, c.N, c.K, c.layout
    ldc, ldaux, ldr, ldd = c.lds()
    if c.trans:  # K-outer operands: [K, ceil8(M)] / [K, ceil8(N)]
        A = torch.zeros((K, -(-M // 8) * 8), dtype=c.in_dt)
        B = torch.zeros((K, -(-N // 8) * 8), dtype=c.in_dt)
        A[:, :M], B[:, :N] = x.A.t(), x.B.t()
        A, B = A.to(dev), B.to(dev)
    else:
        A, B = x.A.to(dev), x.B.to(dev)
    Cbuf, C = _padded(x.C0 if c.beta else (M, N, c.c_dt), ldc, lay.off, dev)
    kw = dict(c.kw, alpha=c.alpha, beta=c.beta, M=M, N=N, K=K)
    watched = [(Cbuf, "C")]
    aux = None
    if c.bias:
        kw["bias"] = x.bias.to(dev)
    if c.aux:
        auxbuf, aux = _padded((M, N, c.c_dt), ldaux, lay.off, dev)
        kw["aux"] = aux
        watched.append((auxbuf, "aux"))
    if c.resid:
        rbuf, kw["resid"] = _padded(x.resid, ldr, lay.off, dev)
        watched.append((rbuf, "resid"))
    if c.dact:
        dbuf, kw["dact_src"] = _padded(x.dsrc, ldd, lay.off, dev)
        watched.append((dbuf, "dact_src"))
        kw["dact"] = c.dact
    else:
        kw["act"] = c.act
    if c.m_dev:
        kw["m_dev"] = torch.tensor([c.live], dtype=torch.int32, device=dev)
        kw["m_hint"] = c.live
    before = [b.clone() for b, _ in watched]
    names = _run(lambda: ops.gemm(A, B, C, **kw))
    torch.cuda.synchronize()
    assert names == [c.kernel()], (c.name, names, c.kernel())
    w = R.check(c, C.cpu(), None if aux is None else aux.cpu(), parts=True)
    # what must survive: everything outside the live rows' N columns of the outputs, all of the inputs
    for (buf, what), b0 in zip(watched, before):
        if what in ("C", "aux"):
            keep = torch.ones(buf.shape, dtype=torch.bool, device=dev)
            keep[:c.live, lay.off:lay.off + N] = False
            assert torch.equal(buf[keep], b0[keep]), f"{c.name}: {what} written outside its live elements"
        else:
            assert torch.equal(buf, b0), f"{c.name}: {what} modified"
    return w


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_epilogue_per_element(dev, family):
    worst = {}
    for c in CASES:
        if c.family == family:
            try:
                worst[c] = _run_case(c, dev)
            except AssertionError:
                raise
            except Exception as e:  # a launch or device error: nothing more runs on this device
                pytest.exit(f"{c.name}: {type(e).__name__}: {e}", returncode=3)
            print(f"{c.name}: worst ratio C {worst[c][0]:.3f} aux {worst[c][1]:.3f}")
    wide = [v[0] for k, v in worst.items() if k.c_dt == torch.float32]
    print(f"family {family}: worst ratio {max(max(v) for v in worst.values()):.3f} over {len(worst)} launches"
          + (f"; C of the fp32-C launches {max(wide):.3f}" if wide else ""))
    bad = {k.name: v for k, v in worst.items() if not max(v) <= 1.0}
    assert not bad, bad
