"""The device schedule the four frozen pre-LN encoder towers share: the CLIP vision tower (clip.ClipCore), ViT
(vit.ViTCore), DINOv3 (dino.DinoCore) and the CLIP text tower (clip_text.ClipTextCore).

`EncoderCore` holds, once, the conversion of the weights into GEMM layout, the per-layer weight builder, the layer
buffers and the layer loop (LN1 -> QKV GEMM -> attention -> out-proj + resid -> LN2 -> fc1 + act -> fc2 + resid, its
LayerNorm-fold variant, and the last layer's "pooled rows only" tail). `ImageEncoderCore` adds what the three image
towers share: the patch-embedding front, the per-batch workspace and `features`. A tower's own file keeps its
modules and key layout, the parameters of its embedding front, its head, and (text) its capped buffers and chunking.
tests/golden/tower_traces.json pins every launch of every tower's `features` (tools/tower_trace.py).
"""

from __future__ import annotations

from types import SimpleNamespace
from typing import Optional

import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from .gpt2 import fold_layernorm

Tensor = torch.Tensor


def cached_core(tower: nn.Module, cls, dtype: torch.dtype):
    """`tower.core(dtype)`: the tower's core of class `cls`, built once per (dtype, device)."""
    key = (dtype, tower.device)
    if getattr(tower, "_core", None) is None or tower._core_key != key:
        tower._core = cls(tower, dtype)
        tower._core_key = key
    return tower._core


def _wb(lin: nn.Linear):
    return lin.weight.data, lin.bias.data


class EncoderCore:
    """Kernel schedule of one tower in one compute dtype: weights in GEMM layout (`refresh`, the tower's own) and
    the encoder layers over ws.x (`encode`). A tower sets `act` and `causal`, and may override `pre_attention` and
    `pooled_rows`."""

    act: int  # the MLP's activation (L.ACT_*), fused into fc1's epilogue
    causal = False

    def __init__(self, m: nn.Module, dtype: torch.dtype):
        self.m, self.dtype = m, dtype
        self.dev = m.device
        L.require_device(self.dev)
        c = m.config
        self.c = c
        self.D, self.H = c.hidden_size, c.num_attention_heads
        self.hd = self.D // self.H
        # LayerNorm 1 (layers >= 1) / LayerNorm 2 (all but the last) folded into the QKV / fc1 tile GEMMs, the row
        # statistics handed over from the producing GEMMs' epilogues (icap_gemm_args.ln_stats_out / ln_stats_in).
        # Only the CLIP vision tower switches it on (ClipCore.refresh)
        self.fold = False
        self._ws = {}
        self.refresh()

    def _cvt(self, t: Tensor) -> Tensor:
        """`t` as a contiguous 2-D operand [t.shape[0], -1] in the compute dtype."""
        t2 = t.reshape(t.shape[0], -1)
        if self.dtype == torch.float32:
            return t2.contiguous()
        out = torch.empty(t2.shape, dtype=self.dtype, device=self.dev)
        ops.convert(t2.contiguous(), out)
        return out

    def _empty(self, *shape, dtype: Optional[torch.dtype] = None) -> Tensor:
        return torch.empty(shape, dtype=dtype or self.dtype, device=self.dev)

    def layer_weights(self, q: nn.Linear, k: nn.Linear, v: nn.Linear, out: nn.Linear, fc1: nn.Linear, fc2: nn.Linear,
                      ln1: nn.LayerNorm, ln2: nn.LayerNorm, out_scale: Optional[Tensor] = None,
                      fc2_scale: Optional[Tensor] = None) -> SimpleNamespace:
        """One layer in GEMM layout: q / k / v fused into one [3D, D] product (a key projection without a bias gets
        a zero one), weights in the compute dtype, biases and LayerNorm parameters fp32. out_scale / fc2_scale: a
        per-channel LayerScale folded into the rows of that projection (lambda * (W x + b) = (lambda W) x + lambda b),
        so it costs nothing per input."""
        w = SimpleNamespace()
        qkv32 = torch.cat([q.weight.data, k.weight.data, v.weight.data], 0)
        k_bias = torch.zeros_like(q.bias.data) if k.bias is None else k.bias.data
        w.qkv_w = self._cvt(qkv32)
        w.qkv_b = torch.cat([q.bias.data, k_bias, v.bias.data], 0).contiguous()
        for name, lin, scale in (("out", out, out_scale), ("fc1", fc1, None), ("fc2", fc2, fc2_scale)):
            wt, b = _wb(lin)
            if scale is not None:
                wt, b = wt * scale[:, None], b * scale
            setattr(w, name + "_w", self._cvt(wt))
            setattr(w, name + "_b", b.contiguous())
        w.ln1, w.ln2 = _wb(ln1), _wb(ln2)
        if self.fold:  # LayerNorm 1 / 2 folded into the QKV / fc1 weights (frozen tower: once)
            w.qkv_wf, w.qkv_ws, w.qkv_bf = fold_layernorm(qkv32, w.ln1[0], w.ln1[1], w.qkv_b, self.dtype)
            w.fc1_wf, w.fc1_ws, w.fc1_bf = fold_layernorm(fc1.weight.data, w.ln2[0], w.ln2[1], w.fc1_b, self.dtype)
        return w

    def layer_buffers(self, M: int, B: int) -> SimpleNamespace:
        """What `encode` works in: M token rows, B pooled rows."""
        D, e = self.D, self._empty
        ws = SimpleNamespace(B=B, M=M)
        ws.x, ws.h1, ws.a, ws.o = e(M, D), e(M, D), e(M, D), e(M, D)
        ws.qkv = e(M, 3 * D)
        ws.f = e(M, self.c.intermediate_size)
        ws.xc = e(B, D)  # the last layer's pooled rows (see encode)
        ws.st_x = ws.st_h = None
        if self.fold:  # (mean, M2) per row and 32-column group of x / h1 (the LayerNorm statistics hand-off)
            ws.st_x = e(M, D // 32, 2, dtype=torch.float32)
            ws.st_h = e(M, D // 32, 2, dtype=torch.float32)
        return ws

    def pre_attention(self, ws, S: int) -> None:
        """Between a layer's QKV GEMM and its attention (DINOv3: the rotary embedding)."""

    def pooled_rows(self, ws, S: int):
        """(o, x, h1, a, f): the attention output and the residual stream of the one row per sequence that reaches
        the output, and the buffers the rest of the last layer runs in — B rows each."""
        raise NotImplementedError

    def encode(self, ws, S: int) -> Tensor:
        """The encoder layers over ws.x (ws.B sequences of S rows); returns ws.xc, the pooled rows after the last
        layer. Only those rows reach a tower's output, and every other row's keys / values are used by the last
        layer's attention, so past that attention the last layer — out-proj, LayerNorm 2, the MLP — runs on the B
        pooled rows alone (`pooled_rows`)."""
        eps, act = self.c.layer_norm_eps, self.act
        scale = self.hd ** -0.5
        fold = ws.st_x is not None
        last = len(self.layers) - 1
        for i, w in enumerate(self.layers):
            if fold and i > 0:  # x's statistics come from the previous layer's fc2 epilogue
                ops.gemm(ws.x, w.qkv_wf, ws.qkv, bias=w.qkv_bf, ln_fold=(w.qkv_ws, eps), ln_stats_in=ws.st_x)
            else:
                ops.layernorm_fwd(ws.x, w.ln1[0], w.ln1[1], eps, ws.a, None, None)
                ops.gemm(ws.a, w.qkv_w, ws.qkv, bias=w.qkv_b)
            self.pre_attention(ws, S)
            ops.attention_fwd(ws.qkv, ws.o, B=ws.B, S=S, H=self.H, hd=self.hd, scale=scale, causal=self.causal)
            if fold and i < last:
                ops.gemm(ws.o, w.out_w, ws.h1, bias=w.out_b, resid=ws.x, ln_stats_out=ws.st_h)
                ops.gemm(ws.h1, w.fc1_wf, ws.f, bias=w.fc1_bf, act=act, ln_fold=(w.fc1_ws, eps), ln_stats_in=ws.st_h)
                ops.gemm(ws.f, w.fc2_w, ws.x, bias=w.fc2_b, resid=ws.h1, ln_stats_out=ws.st_x)
                continue
            o, x, h1, a, f = (ws.o, ws.x, ws.h1, ws.a, ws.f) if i < last else self.pooled_rows(ws, S)
            ops.gemm(o, w.out_w, h1, bias=w.out_b, resid=x)
            ops.layernorm_fwd(h1, w.ln2[0], w.ln2[1], eps, a, None, None)
            ops.gemm(a, w.fc1_w, f, bias=w.fc1_b, act=act)
            ops.gemm(f, w.fc2_w, x if i < last else ws.xc, bias=w.fc2_b, resid=h1)
        return ws.xc


class ImageEncoderCore(EncoderCore):
    """An image tower: S = NP prefix rows (CLS, registers) + G * G patch rows per image, the CLS row pooled. The
    tower gives `refresh` (which calls `patch_weights`), `alloc_head`, `embed` (the front, into ws.x) and `head`
    (ws.xc -> ws.emb), and names in `raw` the workspace field that holds its un-normalised features."""

    raw = "pool"

    def __init__(self, m: nn.Module, dtype: torch.dtype):
        c = m.config
        self.G = c.image_size // c.patch_size
        self.NP = 1 + getattr(c, "num_register_tokens", 0)
        self.S = self.G * self.G + self.NP
        super().__init__(m, dtype)

    def patch_weights(self, conv: nn.Conv2d, prefix: Tensor, pos: Optional[Tensor] = None,
                      fused: Optional[bool] = None) -> None:
        """The patch-embedding front's operands: the Conv2d(stride = kernel = patch) weight as [D, C*p*p] in
        (c, ky, kx) order, zero-padded to the 8-multiple row of icap_im2col_patches (p = 14: 592), its bias (or
        None), the fp32 prefix rows [NP, D] and position table [S, D] (or None). fused: run the front as the one
        gather GEMM that reads the pixels itself (icap_patch_embed, bf16 only) — by default wherever it exists."""
        wp = conv.weight.data.reshape(self.D, -1)
        self.Kp = (wp.shape[1] + 7) // 8 * 8
        if self.Kp != wp.shape[1]:
            wp = torch.nn.functional.pad(wp, (0, self.Kp - wp.shape[1]))
        self.w_patch = self._cvt(wp)
        self.b_patch = None if conv.bias is None else conv.bias.data.contiguous()
        self.prefix, self.pos = prefix.reshape(self.NP, self.D).contiguous(), pos
        self.fused_patch = self.dtype == torch.bfloat16 if fused is None else fused

    def embed_patches(self, ws, pixels: Tensor, x: Tensor) -> None:
        """x[b] = [prefix rows || patch embeddings of image b] (+ positions)."""
        c, D, B, G2 = self.c, self.D, ws.B, self.G * self.G
        if self.fused_patch:
            # Conv2d + prefix rows + positions in one launch that gathers the pixel runs into its LDS stages (no
            # im2col patch matrix, no separate embedding pass)
            ops.patch_embed(pixels, self.w_patch, x, patch=c.patch_size, prefix=self.prefix, pos=self.pos,
                            bias=self.b_patch)
            return
        ops.im2col_patches(pixels, ws.patches, c.patch_size)  # the im2col matrix and the GEMM over it
        ops.gemm(ws.patches, self.w_patch, ws.pe, bias=self.b_patch)  # Conv2d(stride=patch) as a GEMM
        if self.pos is None:
            ops.prefix_embed(ws.pe, self.prefix, x, B, G2, D)
        else:  # (the towers with a position table have the CLS row alone in front)
            ops.vit_embed(ws.pe, self.prefix, self.pos, x, B, G2, D)

    def alloc(self, B: int) -> SimpleNamespace:
        if B in self._ws:
            return self._ws[B]
        ws = self.layer_buffers(B * self.S, B)
        if not self.fused_patch:  # (icap_patch_embed reads the pixels itself — no patch matrix)
            ws.patches = self._empty(B * self.G * self.G, self.Kp)
            ws.pe = self._empty(B * self.G * self.G, self.D)
        self.alloc_head(ws)
        self._ws = {B: ws}  # keep only the latest batch size
        return ws

    def alloc_head(self, ws) -> None:
        """The head's buffers (default: the normed CLS rows, then fp32 pooled output and embedding of width D)."""
        ws.cls = self._empty(ws.B, self.D)
        ws.pool = self._empty(ws.B, self.D, dtype=torch.float32)
        ws.emb = self._empty(ws.B, self.D, dtype=torch.float32)

    def pooled_rows(self, ws, S: int):
        # the CLS rows as strided views (row b at b*S*D)
        B, D = ws.B, self.D
        return ws.o.view(B, S * D)[:, :D], ws.x.view(B, S * D)[:, :D], ws.h1[:B], ws.a[:B], ws.f[:B]

    def run(self, ws, pixels: Tensor) -> Tensor:
        """Kernel schedule; fills the tower's un-normalised features and returns ws.emb (fp32, L2-normalised) —
        graph-capturable."""
        self.embed(ws, pixels)
        self.encode(ws, self.S)
        self.head(ws)
        return ws.emb

    @torch.no_grad()
    def features(self, pixels: Tensor, normalize: bool = True) -> Tensor:
        if pixels.dtype != torch.float32 or not pixels.is_contiguous():
            pixels = pixels.float().contiguous()
        ws = self.alloc(pixels.shape[0])
        self.run(ws, pixels)
        return (ws.emb if normalize else getattr(ws, self.raw)).clone()
