"""Regenerates tests/golden/clip_text_plan_cover.json: every launch plan the GEMM planner picks for the CLIP text
tower's schedule (icap.clip_text.ClipTextCore.run) under its caps — each GEMM form of icap.clip_text.schedule_gemms
(qkv, out, fc1, fc2 at every M in 1 ... ROWS_CAP, which includes their pooled-row forms; the projection at every M in
1 ... CAPTIONS_CAP), in bf16 and fp32, at the tiny (test), ViT-B/32 and ViT-L/14 text widths, planned through the
host-only queries icap_gemm_plan_info / icap_gemm_kernel_name with the arguments ops.gemm passes (the usual split-K
workspace and tickets). For each distinct (kernel name, splits, fused) of a (geometry, dtype, kind) it records the
smallest M that plans it: the shapes tests/test_clip_text_gpu.py runs against fp64, so that no kernel the schedule
can launch goes untested. Needs no GPU (the planner assumes 256 compute units without one).

usage: python tools/clip_text_plan_cover.py [output.json]"""

import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpt2-image-captioning_amd"))

from icap import _lib, ops  # noqa: E402
from icap.clip_text import CAPTIONS_CAP, ROWS_CAP, CLIPTextConfig, schedule_gemms  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "clip_text_plan_cover.json")


def geometries():
    """name -> config: the test geometry (tests/clip_text_helpers.py tiny_config) and the two openai text towers"""
    tiny = CLIPTextConfig(vocab_size=512, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
                          intermediate_size=256, max_position_embeddings=77, projection_dim=64)
    return {"tiny": tiny, "b32": CLIPTextConfig(), "l14": CLIPTextConfig.vit_l14()}


def gemm_args(M, N, K, in_dtype, epi):
    """icap_gemm_args as ops.gemm fills them for one launch of the schedule (fake operand pointers: the planner
    never dereferences one)."""
    a = _lib.GemmArgs()
    a.M, a.N, a.K = M, N, K
    a.in_dtype = in_dtype
    a.c_dtype = _lib.F32 if epi.get("c_f32") else in_dtype
    a.A = a.B = a.C = 1 << 20
    a.lda, a.ldb, a.ldc = K, K, N
    a.alpha = 1.0
    if epi.get("bias"):
        a.bias = 1 << 23
    a.act = epi.get("act", _lib.ACT_NONE)
    if epi.get("resid"):
        a.resid, a.ldr = 1 << 24, N
    a.workspace, a.workspace_bytes = 1 << 21, ops.GEMM_WORKSPACE_BYTES
    a.tickets, a.tickets_len = 1 << 22, ops.GEMM_TICKETS
    return a


def record():
    """[{geometry, dtype, kind, N, K, name, splits, fused, M}]: one entry per distinct plan, M the smallest that
    plans it, in the order the sweep meets them."""
    lib = _lib.load()
    splits, fused = C.c_int32(), C.c_int32()
    out = []
    for gname, cfg in geometries().items():
        for dname, dt in (("bf16", _lib.BF16), ("fp32", _lib.F32)):
            for kind, N, K, m_max, epi in schedule_gemms(cfg):
                seen = set()
                for M in range(1, m_max + 1):
                    a = gemm_args(M, N, K, dt, epi)
                    if lib.icap_gemm_plan_info(C.byref(a), C.byref(splits), C.byref(fused)) != 0:
                        raise RuntimeError(f"{gname} {dname} {kind} M={M}: {lib.icap_last_error().decode()}")
                    key = (lib.icap_gemm_kernel_name(C.byref(a)).decode(), splits.value, fused.value)
                    if key not in seen:
                        seen.add(key)
                        out.append({"geometry": gname, "dtype": dname, "kind": kind, "N": N, "K": K, "name": key[0],
                                    "splits": key[1], "fused": key[2], "M": M})
    return out


def dump(plans, f):
    f.write('{"rows_cap": %d, "captions_cap": %d, "plans": [\n' % (ROWS_CAP, CAPTIONS_CAP))
    f.write(",\n".join(json.dumps(p) for p in plans) + "\n]}\n")


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    plans = record()
    with open(path, "w") as f:
        dump(plans, f)
    print(f"{path}: {len(plans)} plans, {os.path.getsize(path)} bytes")
