"""Variant 24 (192 x 64 tiles, ops.gemm(w192=True)) against the automatic plan and hipBLASLt (torch.mm, plain
products only) on the step's N = 768 products, each captured as 20 back-to-back launches in a HIP graph and replayed
5 times (best per-launch us). Forms (diagnostic build, ICAP_LIB=.../libicap_hip_stamps.so, whose switches are read
at capture time): auto = the automatic plan; p7 = path 7 (natural k order: variant 24 up to 16 k-stages, the
4-stage ring variant 25 past that); p7r3 / p7n2 = path 7 with the 3-stage ring / the double-buffered loop for long
K (ICAP_W192R = 3 / 2; forms removed after round 5's third pass: p7r5 = fragment prefetch, p7rs = register staging);
p7s2 / p7s3 = path 7 with K split 2 / 3 ways and combined inside the launch (ICAP_W192S); w192s = the automatic plan
forced to the 192-row tiles with its K-skew. '!' = not allclose to auto; '#' = not bitwise equal to p7."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gpt2-image-captioning_amd"), os.path.dirname(os.path.abspath(__file__))]
import torch  # noqa: E402

from icap import _lib as L  # noqa: E402
from icap import ops  # noqa: E402
from gemm_helpers_ab import names_of  # noqa: E402

dev = torch.device("cuda", 0)
REPS = 20
SHAPES = [  # (M capacity, live rows or None, N, K, epilogue, what)
    (8320, 3584, 768, 768, "resid_drop_lns", "gpt2 attn c_proj fwd (LN stats)"),
    (8320, 3584, 768, 768, "plain", "gpt2 attn c_proj dX"),
    (8320, 3584, 768, 2304, "plain", "gpt2 c_attn dX"),
    (8320, 3584, 768, 3072, "resid_drop", "gpt2 mlp c_proj fwd"),
    (3200, None, 768, 768, "resid_drop", "mapper out_proj fwd"),
    (3200, None, 768, 768, "plain", "mapper 768 dX"),
    (3200, None, 768, 3072, "resid_drop", "mapper linear2 fwd"),
    (6400, None, 768, 768, "resid", "clip out_proj"),
    (6400, None, 768, 3072, "resid", "clip fc2"),
]


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
    for _ in range(5):
        e0.record()
        gr.replay()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / REPS)
    del gr
    return best


g = torch.Generator(device="cpu").manual_seed(0)
FORMS = [("auto", {}, {}), ("p7", {}, dict(w192=True)), ("p7s2", {"ICAP_W192S": "2"}, dict(w192=True)),
         ("p7s3", {"ICAP_W192S": "3"}, dict(w192=True)), ("p7n2", {"ICAP_W192R": "2"}, dict(w192=True))]
print(f"{'shape':48s} " + " ".join(f"{f[0]:>8s}" for f in FORMS) + f" {'hipBLASLt':>10s}   (us per launch, graph replay)")
for M, live, N, K, epi, what in SHAPES:
    rows = live or M
    A = (torch.rand((M, K), generator=g) * 2 - 1).to(dev, torch.bfloat16)
    B = (torch.rand((N, K), generator=g) * 2 - 1).to(dev, torch.bfloat16)
    C = torch.zeros((M, N), device=dev, dtype=torch.bfloat16)
    kw = {}
    if epi.startswith("resid"):
        kw = dict(bias=torch.zeros(N, device=dev), resid=torch.randn((M, N), device=dev).to(torch.bfloat16))
        if "drop" in epi:
            kw["drop"] = ops.Dropout(0.1, 1)
        if epi.endswith("lns"):
            kw["ln_stats_out"] = torch.empty((M, N // 32, 2), device=dev)
    if live is not None:
        kw.update(m_dev=torch.tensor([live], dtype=torch.int32, device=dev), m_hint=live)
    cells, ref, names = [], None, []
    for name, env, extra in FORMS:
        os.environ.update(env)
        try:
            t = per_launch(lambda: ops.gemm(A, B, C, **kw, **extra))
            names.append(names_of(lambda: ops.gemm(A, B, C, **kw, **extra)).replace("gemm_kernel<bf16, bf16, ", "<"))
        finally:
            for k in env:
                os.environ.pop(k, None)
        got = C[:rows].float().clone()
        ref = got if ref is None else ref
        ok = torch.allclose(got, ref, rtol=2e-2, atol=2e-2)
        if name == "p7":
            p7 = got
        mark = " " if ok else "!"
        if name in ("p7n2",) and not torch.equal(got, p7):
            mark = "#"  # not bitwise equal to path 7's default form (same k order: must be equal)
        cells.append(f"{t:7.1f}{mark}")
    lib = ""
    if epi == "plain":
        a = A[:rows]
        lib = f"{per_launch(lambda: torch.mm(a, B.t(), out=C[:rows])):10.1f}"
    print(f"{what + f' {rows}x{N}x{K}':48s} " + " ".join(cells) + f" {lib:>10s}   " + " | ".join(names), flush=True)
