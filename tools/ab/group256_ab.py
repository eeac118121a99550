"""Round 10: the grouped weight-gradient launch (icap_gemm_group) on 128 x 256 tiles against the 128 x 128 body
(ICAP_GROUP128=1, read at every grouped call), at the mapper's shapes over 3200 token rows.

  python tools/ab/group256_ab.py            timing: each group captured as 20 back-to-back launches in a HIP graph,
                                            replayed 7 times, best per-launch us; outputs compared bitwise
  python tools/ab/group256_ab.py stamps     phase stamps of one launch of the layer's group per body (diagnostic build:
                                            make -C gpt2-image-captioning_amd/csrc stamps; a block that walks two tiles
                                            leaves the stamps of its last one, so its start is the first tile's length)
With ICAP_LIB set to the diagnostic build, ICAP_GEMM_DIAG=1 / 2 / 3 drops the A / B / both operands' staging loads from
the timing (zero-record descriptors: the instruction stream, waits and barriers stay; the outputs are zeros): what is
left of a k-step is the LDS reads, the MFMAs and the barriers.
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
STAMPS = len(sys.argv) > 1 and sys.argv[1] == "stamps"
if STAMPS:
    os.environ.setdefault("ICAP_LIB", os.path.join(ROOT, "gpt2-image-captioning_amd", "icap", "libicap_hip_stamps.so"))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gpt2-image-captioning_amd"), os.path.dirname(os.path.abspath(__file__))]
import torch  # noqa: E402

from icap import _lib as L  # noqa: E402
from icap import ops  # noqa: E402

dev = torch.device("cuda", 0)
ROWS = 3200
REPS = 20
LAYER = [("linear1", 3072, 768), ("linear2", 768, 3072), ("in_proj", 2304, 768), ("out_proj", 768, 768)]


def per_launch(body):
    body()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with ops.graph_capture(gr):
        for _ in range(REPS):
            body()
    gr.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e9
    for _ in range(7):
        e0.record()
        gr.replay()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / REPS)
    del gr
    return best


def products(names, bias, g):
    ones = torch.ones((ROWS, 8), device=dev, dtype=torch.bfloat16)
    items = []
    for name, M, N in LAYER:
        if name not in names:
            continue
        dY = (torch.randn((ROWS, M), generator=g) * 0.2).to(dev, torch.bfloat16)
        X = torch.randn((ROWS, N), generator=g).to(dev, torch.bfloat16)
        items.append((dY, X, torch.zeros((M, N), device=dev), M, N, ROWS, 0.0))
    if bias:
        items += [(it[0], ones, torch.zeros((it[3], 1), device=dev), it[3], 1, ROWS, 0.0) for it in list(items)]
    return items


def tiles(items, big):
    if big:
        return sum(-(-it[3] // 256) if it[4] <= 4 else -(-it[3] // 128) * -(-it[4] // 256) for it in items)
    return sum(-(-it[3] // 128) * -(-it[4] // 128) for it in items)


def run(items, force128):
    if force128:
        os.environ["ICAP_GROUP128"] = "1"
    try:
        t = per_launch(lambda: ops.gemm_group(items))
    finally:
        os.environ.pop("ICAP_GROUP128", None)
    torch.cuda.synchronize()
    return t, [it[2].clone() for it in items]


def timing():
    g = torch.Generator(device="cpu").manual_seed(0)
    nk = (ROWS + 63) // 64
    print(f"{'group':40s} {'tiles128':>8s} {'us':>7s} {'tiles256':>8s} {'us':>7s} {'us/kstep (one round)':>21s}  bitwise")
    for what, names, bias in [("linear1 3072x768x3200", ("linear1",), False),
                              ("linear2 768x3072x3200", ("linear2",), False),
                              ("layer: 4 dW", [n for n, _, _ in LAYER], False),
                              ("layer: 4 dW + 4 bias sums", [n for n, _, _ in LAYER], True)]:
        items = products(names, bias, g)
        t_old, o_old = run(items, True)
        t_new, o_new = run(items, False)
        same = all(torch.equal(a, b) for a, b in zip(o_old, o_new))
        n_old, n_new = tiles(items, False), tiles(items, True)
        ks = f"{t_new / nk:.3f}" if n_new <= 256 else "-"
        ko = f"{t_old / nk:.3f}" if n_old <= 256 else "-"
        print(f"{what:40s} {n_old:8d} {t_old:7.1f} {n_new:8d} {t_new:7.1f} {'128: ' + ko + '  256: ' + ks:>21s}  "
              f"{'equal' if same else 'DIFFERENT'}", flush=True)


def stamps():
    g = torch.Generator(device="cpu").manual_seed(0)
    items = products([n for n, _, _ in LAYER], True, g)
    st = torch.zeros(8 * 1024, dtype=torch.int64, device=dev)
    n = len(items)
    arr = (L.GemmArgs * n)()
    for i, (A, B, out, M, N, K, beta) in enumerate(items):
        a = arr[i]
        a.trans_ab = 1
        a.M, a.N, a.K = M, N, K
        a.in_dtype, a.c_dtype = L.BF16, L.F32
        a.A, a.lda, a.B, a.ldb, a.C, a.ldc = A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), out.data_ptr(), out.stride(0)
        a.alpha, a.beta, a.split_k = 1.0, beta, 1
        a.diag_stamps = st.data_ptr()
    med = lambda xs: statistics.median(xs) if xs else 0.0  # noqa: E731
    nk = (ROWS + 63) // 64
    print(f"{'body':10s} {'blocks':>6s} {'span':>6s} {'start: min/50/max':>18s} {'late starts':>11s} {'prolog':>6s} "
          f"{'loop':>6s} {'/kstep':>6s} {'epil':>5s}  (us; the last tile of each block)")
    for body, force in (("128x128", True), ("128x256", False)):
        if force:
            os.environ["ICAP_GROUP128"] = "1"
        try:
            for _ in range(5):
                ops.call("icap_gemm_group", arr, n, ops._stream())
            st.zero_()
            torch.cuda.synchronize()
            ops.call("icap_gemm_group", arr, n, ops._stream())
            torch.cuda.synchronize()
        finally:
            os.environ.pop("ICAP_GROUP128", None)
        rows = [r for r in st.view(-1, 8).cpu().tolist() if r[1] != 0]
        t0 = min(r[1] for r in rows)
        starts = sorted((r[1] - t0) * 0.01 for r in rows)
        ends = [(r[5] - t0) * 0.01 for r in rows]
        prolog = [(r[2] - r[1]) * 0.01 for r in rows]
        loop = [(r[3] - r[2]) * 0.01 for r in rows]
        epil = [(r[5] - r[4]) * 0.01 for r in rows]
        late = sum(1 for s in starts if s > 10.0)  # blocks whose stamped tile began after a first one
        print(f"{body:10s} {len(rows):6d} {max(ends):6.1f} {starts[0]:5.1f}/{med(starts):5.1f}/{starts[-1]:5.1f} {late:11d} "
              f"{med(prolog):6.2f} {med(loop):6.2f} {med(loop) / nk:6.3f} {med(epil):5.2f}", flush=True)


if __name__ == "__main__":
    stamps() if STAMPS else timing()
