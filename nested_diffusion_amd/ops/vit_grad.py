"""The backward chain of the ViT: the input gradient of each forward piece and the cross-entropy head.  Binds csrc/nd_vit_grad.hip
(include/nested_diffusion.h: "input gradient of the full ViT and the Linf attacks"); nd_margin_head_bwd of that unit is bound in
attack_l2."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from .. import _lib
from .._lib import check, ptr
from ._base import _f32, _image_or_tensor, _labels, _opt_f32, _stream
from .gemm import SplitMatrix


def layernorm_grad(x: torch.Tensor, weight: torch.Tensor, g: torch.Tensor, eps: float, residual: Optional[torch.Tensor] = None,
                   want_out: bool = True, want_split: bool = False):
    """Input gradient of LayerNorm(x) * weight + bias given g = dL/d(output), plus `residual` (the gradient the residual stream carries
    past the LayerNorm).  mean / rstd are recomputed from x.  Returns fp32 [rows, dim], its frag32b3 image (want_split), or both."""
    x, g = _f32(x, "x"), _f32(g, "g")
    if g.shape != x.shape:
        raise ValueError(f"g is {tuple(g.shape)}, x is {tuple(x.shape)}")
    residual = _opt_f32(residual, "residual")
    if residual is not None and residual.shape != x.shape:
        raise ValueError("residual must have the shape of x")
    if not (want_out or want_split):
        raise ValueError("nothing to return")
    dim = x.shape[-1]
    rows = x.numel() // dim
    out = torch.empty_like(x) if want_out else None
    osp = SplitMatrix(rows, dim, x.device) if want_split else None
    check(_lib.load().nd_layernorm_bwd(ptr(x), ptr(_f32(weight, "weight")), ptr(g), ptr(residual), ptr(out), ptr(osp.data) if osp else None,
                                       rows, dim, float(eps), _stream(x)), "nd_layernorm_bwd")
    return _image_or_tensor(out, osp, want_out, want_split)


def gelu_split(u: torch.Tensor, want_out: bool = False):
    """GELU(u) (exact erf, the expression of the fc1 epilogue) written as the frag32b3 image of [rows, cols] (and fp32 with want_out)."""
    u = _f32(u, "u")
    rows, cols = u.shape
    out = torch.empty_like(u) if want_out else None
    osp = SplitMatrix(rows, cols, u.device)
    check(_lib.load().nd_gelu_split(ptr(u), ptr(out), ptr(osp.data), rows, cols, _stream(u)), "nd_gelu_split")
    return _image_or_tensor(out, osp, want_out, True)


def gelu_grad_split(u: torch.Tensor, dg: torch.Tensor, want_out: bool = False):
    """dg * GELU'(u) as the frag32b3 image of [rows, cols] (and fp32 with want_out)."""
    u, dg = _f32(u, "u"), _f32(dg, "dg")
    if dg.shape != u.shape:
        raise ValueError(f"dg is {tuple(dg.shape)}, u is {tuple(u.shape)}")
    rows, cols = u.shape
    out = torch.empty_like(u) if want_out else None
    osp = SplitMatrix(rows, cols, u.device)
    check(_lib.load().nd_gelu_bwd_split(ptr(u), ptr(dg), ptr(out), ptr(osp.data), rows, cols, _stream(u)), "nd_gelu_bwd_split")
    return _image_or_tensor(out, osp, want_out, True)


ATTENTION_BWD_MAX_TOKENS = 208      # ATB_NMAX of csrc/nd_vit_grad.hip: the keys per (image, head) k_attention_bwd holds in LDS


def attention_grad(qkv: torch.Tensor, o: torch.Tensor, dout: torch.Tensor, B: int, N: int, heads: int, want_out: bool = True,
                   want_split: bool = False):
    """dqkv [B*N, 3*heads*64] of o = softmax(q k^T / 8) v (timm layout) given dout = dL/do; fp32, its frag32b3 image, or both."""
    qkv, o, dout = _f32(qkv, "qkv"), _f32(o, "o"), _f32(dout, "dout")
    if tuple(qkv.shape) != (B * N, 3 * heads * 64) or tuple(o.shape) != (B * N, heads * 64) or dout.shape != o.shape:
        raise ValueError(f"qkv {tuple(qkv.shape)}, o {tuple(o.shape)}, dout {tuple(dout.shape)} do not match B={B}, N={N}, heads={heads}")
    if not (want_out or want_split):
        raise ValueError("nothing to return")
    out = torch.empty_like(qkv) if want_out else None
    osp = SplitMatrix(B * N, 3 * heads * 64, qkv.device) if want_split else None
    check(_lib.load().nd_attention_bwd(ptr(qkv), ptr(o), ptr(dout), ptr(out), ptr(osp.data) if osp else None, B, N, heads, _stream(qkv)),
          "nd_attention_bwd")
    return _image_or_tensor(out, osp, want_out, want_split)


def xent_head_grad(logits: torch.Tensor, labels: torch.Tensor, head_w: torch.Tensor,
                   check_labels: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dfeat [B, E] = (softmax(logits) - onehot(labels)) . head_w, per-image cross-entropy [B]): the gradient of
    crossentropy(logits, labels).sum() with respect to the head's input.  check_labels=False skips the label-range check, the call's only
    read-back."""
    logits, head_w = _f32(logits, "logits"), _f32(head_w, "head_w")
    B, C = logits.shape
    if head_w.dim() != 2 or head_w.shape[0] != C:
        raise ValueError(f"head_w is {tuple(head_w.shape)}, logits {tuple(logits.shape)}")
    labels = _labels(labels, logits.device, B, C if check_labels else None)
    E = head_w.shape[1]
    dfeat = torch.empty(B, E, dtype=torch.float32, device=logits.device)
    loss = torch.empty(B, dtype=torch.float32, device=logits.device)
    check(_lib.load().nd_xent_head_bwd(ptr(logits), ptr(labels), ptr(head_w), ptr(dfeat), ptr(loss), B, C, E, _stream(logits)),
          "nd_xent_head_bwd")
    return dfeat, loss


def unpatchify(cols: torch.Tensor, B: int, Cin: int, H: int, W: int, p: int) -> torch.Tensor:
    """[B*(H/p)*(W/p), Cin*p*p] -> [B, Cin, H, W]: the exact inverse of patchify."""
    cols = _f32(cols, "cols")
    if H % p or W % p or tuple(cols.shape) != (B * (H // p) * (W // p), Cin * p * p):
        raise ValueError(f"cols is {tuple(cols.shape)}; expected [{B * (H // p) * (W // p)}, {Cin * p * p}]")
    img = torch.empty(B, Cin, H, W, dtype=torch.float32, device=cols.device)
    check(_lib.load().nd_unpatchify(ptr(cols), ptr(img), B, Cin, H, W, p, _stream(cols)), "nd_unpatchify")
    return img
