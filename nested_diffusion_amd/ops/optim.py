"""The fused gradient + optimizer steps of the mapping MLPs and the ViT, and the ensemble head they train against.  Binds
csrc/nd_mlp_train.hip, csrc/nd_vit_train.hip and nd_ensemble_xent_bwd of csrc/nd_mlp_grad.hip (include/nested_diffusion.h: "the gradient
through the mapping MLPs", "training of the mapping MLPs", "training of the ViT"; the loops: train_mapping.py, train_transformer.py)."""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Tuple

import torch

from .. import _lib
from .._lib import check, ptr
from ._base import _f32, _inplace, _labels, _on, _stream, _workspace
from .packed_linear import LINEAR_BWD_MAX_M, PackedWeight


def ensemble_xent_grad(logits: torch.Tensor, labels: Optional[torch.Tensor] = None, check_labels: bool = True):
    """(P [B, C], loss [B], dlogits [K, B, C]) of the cross-entropy of the members' averaged softmax (nd_ensemble_xent_bwd): logits
    [K, B, C], P = mean_k softmax(logits_k), loss = -log P[b, label], dlogits_k = dloss / dlogits_k.  labels None: (P, None, None), the
    scores-only call.  check_labels=False skips the label-range check, which reads back (the kernel gives an out-of-range label a NaN loss
    and no gradient)."""
    logits = _f32(logits, "logits")
    if logits.dim() != 3:
        raise ValueError("logits must be [K, B, C]")
    K, B, C = logits.shape
    if not 1 <= K <= 32 or B < 1 or not 2 <= C <= 1024:
        raise ValueError(f"the ensemble head takes 1 <= K <= 32 members, B >= 1 and 2 <= C <= 1024 classes (K={K}, B={B}, C={C})")
    P = torch.empty(B, C, dtype=torch.float32, device=logits.device)
    loss = dlogits = None
    if labels is not None:
        labels = _labels(labels, logits.device, B, C if check_labels else None)
        loss = torch.empty(B, dtype=torch.float32, device=logits.device)
        dlogits = torch.empty_like(logits)
    check(_lib.load().nd_ensemble_xent_bwd(ptr(logits), ptr(labels), ptr(P), ptr(loss), ptr(dlogits), K, B, C, _stream(logits)),
          "nd_ensemble_xent_bwd")
    return P, loss, dlogits


def _adam_fields(what: str, lr: float, t: int, betas: Tuple[float, float], eps: float) -> tuple:
    """The seven fields nd_adam_step and nd_adamw_step share, formed in double, as torch's Python does (ctypes rounds each to fp32 once):
    step_size = lr / (1 - beta1^t), sqrt_bc2 = sqrt(1 - beta2^t)."""
    t = int(t)
    if t < 1:
        raise ValueError(f"{what}: steps count from 1 (t={t})")
    b1, b2 = float(betas[0]), float(betas[1])
    if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0) or lr < 0.0 or eps < 0.0:
        raise ValueError(f"{what} needs lr >= 0, eps >= 0 and betas in [0, 1) (lr={lr}, betas={betas}, eps={eps})")
    return b1, 1.0 - b1, b2, 1.0 - b2, float(lr) / (1.0 - b1 ** t), (1.0 - b2 ** t) ** 0.5, float(eps)


def adam_step(lr: float, t: int, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8) -> "_lib.NdAdamStep":
    """nd_adam_step of step t >= 1 (torch.optim.Adam's `step` after its increment)."""
    return _lib.NdAdamStep(*_adam_fields("adam_step", lr, t, betas, eps))


def adamw_step(lr: float, t: int, weight_decay: float = 0.1, betas: Tuple[float, float] = (0.9, 0.999),
               eps: float = 1e-8) -> "_lib.NdAdamwStep":
    """nd_adamw_step of step t >= 1 (torch.optim.AdamW's `step` after its increment): adam_step's fields plus decay = 1 - lr *
    weight_decay, formed in double like them."""
    if weight_decay < 0.0:
        raise ValueError(f"adamw_step needs weight_decay >= 0 (weight_decay={weight_decay})")
    return _lib.NdAdamwStep(*_adam_fields("adamw_step", lr, t, betas, eps), 1.0 - float(lr) * float(weight_decay))


def ema_step(mu: float) -> "_lib.NdEmaStep":
    """nd_ema_step of the rate mu in (0, 1) (diffusion/ema.py EMA(mu)): 1 - mu is formed in double, as Python forms `1. - self.mu`, and
    each coefficient is rounded to fp32 once -- (float)(1.0 - mu), not 1.0f - (float)mu."""
    mu = float(mu)
    if not (math.isfinite(mu) and 0.0 < mu < 1.0):
        raise ValueError(f"ema_step needs a finite rate with 0 < mu < 1 (mu={mu})")
    return _lib.NdEmaStep(1.0 - mu, mu)


_STEP_ARG = {_lib.NdAdamStep: "adam", _lib.NdAdamwStep: "adamw"}


def _fused_state(step, step_type, return_grad: bool, what: str, dev, state) -> bool:
    """The checks every gradient + optimizer call shares; True when the call is fused.  step: the call's ops.adam_step / ops.adamw_step
    (a step_type), or None for the gradient-only call, which then needs return_grad.  state: (tensor-or-image, name, size) of every
    buffer the update writes in place, all distinct: a float32 contiguous tensor on `dev` of shape `size` (a tuple) or of `size` elements
    (an int), or -- `size` a PackedWeight -- a PackedWeight image of its (N, K, dtype, device)."""
    arg = _STEP_ARG[step_type]
    if step is None:
        if not return_grad:
            raise ValueError(f"{what}: {arg}=None and return_grad=False: nothing to compute")
        return False
    if not isinstance(step, step_type):
        raise TypeError(f"{arg} must be an ops.{arg}_step(...) or None")
    ptrs = set()
    for t, name, size in state:
        if isinstance(size, PackedWeight):
            if not isinstance(t, PackedWeight):
                raise TypeError(f"{name} must be a PackedWeight (weight.zeros_like())")
            if (t.N, t.K, t.dtype) != (size.N, size.K, size.dtype) or t.data.device != size.data.device:
                raise ValueError(f"{name} is a [{t.N}, {t.K}] image on {t.data.device}; expected weight's [{size.N}, {size.K}] on "
                                 f"{size.data.device}")
            t = t.data
        else:
            if t is None:
                raise ValueError(f"{what}: {name} is None in a fused call")
            shaped = isinstance(size, tuple)
            _inplace(t, name, shape=size if shaped else None)
            if (not shaped and t.numel() != size) or t.device != dev:
                raise ValueError(f"{name} has {t.numel()} elements on {t.device}; expected {size} on {dev}")
        ptrs.add(t.data_ptr())
    if len(ptrs) != len(state):
        raise ValueError(f"{what}: the parameter and moment buffers must be distinct")
    return True


def linear_wgrad_adam(dy: torch.Tensor, x: torch.Tensor, weight: PackedWeight, m: Optional[PackedWeight], v: Optional[PackedWeight], adam,
                      gscale: float = 1.0, return_grad: bool = False) -> Optional[PackedWeight]:
    """One Adam step of linear(x, weight)'s weight on the gradient gscale * (dy^T @ x), dy = dL/d(its output) [M, N], x its input [M, K]
    (nd_linear_wgrad_adam: the gradient is formed tile by tile and applied in registers, never written unless asked for).  weight, m, v
    are updated IN PLACE in their packed images: weight.data keeps its address, so whatever streams that image sees the new weights.
    adam: ops.adam_step(lr, t), or None for the gradient-only call (m, v unused).  return_grad: also return the gradient as a packed
    image (.unpack() gives [N, K]).  1 <= M <= 128."""
    lib = _lib.load()
    if not isinstance(weight, PackedWeight):
        raise TypeError("weight must be a PackedWeight (the image the forward streams)")
    if weight.dtype != _lib.ND_DTYPE_F32:
        raise _lib.NdError("linear_wgrad_adam updates fp32 weight images only: training runs in fp32 mode, not on an fp16 PackedWeight")
    dy, x = _f32(dy, "dy"), _f32(x, "x")
    if dy.dim() != 2 or dy.shape[0] < 1 or dy.shape[1] != weight.N:
        raise ValueError(f"dy is {tuple(dy.shape)}, weight is [{weight.N}, {weight.K}]: expected [M >= 1, {weight.N}]")
    M, N, K = dy.shape[0], weight.N, weight.K
    if M > LINEAR_BWD_MAX_M:
        raise ValueError(f"linear_wgrad_adam takes at most {LINEAR_BWD_MAX_M} rows per step (M={M}): a weight gradient sums over the batch, "
                         f"it cannot run as chunks")
    if K % 16:
        raise ValueError(f"K must be a multiple of 16 (K={K})")
    _on(x, "x", (M, K), dy.device)
    if weight.data.device != dy.device:
        raise ValueError(f"weight is on {weight.data.device}, dy on {dy.device}")
    on = _fused_state(adam, _lib.NdAdamStep, return_grad, "linear_wgrad_adam", dy.device, ((weight, "weight", weight), (m, "m", weight), (v, "v", weight)))
    g = weight.zeros_like() if return_grad else None
    check(lib.nd_linear_wgrad_adam(ptr(dy), ptr(x), ptr(weight.data), ptr(m.data) if on else None, ptr(v.data) if on else None,
                                   ptr(g.data) if g is not None else None, M, N, K, weight.dtype, float(gscale),
                                   ctypes.byref(adam) if on else None, _stream(dy)), "nd_linear_wgrad_adam")
    return g


def linear_wgrad_plan(N: int, K: int) -> dict:
    """The launch geometry of nd_linear_wgrad_adam for an [N, K] weight (host only): 16-column blocks per workgroup, workgroups over K,
    workgroups over the row blocks, row blocks per workgroup."""
    out = (ctypes.c_int * 4)()
    check(_lib.load().nd_linear_wgrad_plan(int(N), int(K), out), "nd_linear_wgrad_plan")
    return {"kb_per_wg": out[0], "grid_x": out[1], "grid_y": out[2], "rb_per_wg": out[3]}


def bias_grad_adam(dy: torch.Tensor, bias: torch.Tensor, m: Optional[torch.Tensor], v: Optional[torch.Tensor], adam, gscale: float = 1.0,
                   return_grad: bool = False) -> Optional[torch.Tensor]:
    """One Adam step of a bias [N] on the gradient gscale * dy.sum(0) (summed in the order m = 0 .. M - 1), in place (nd_bias_grad_adam).
    adam None: the gradient-only call."""
    dy = _f32(dy, "dy")
    if dy.dim() != 2 or dy.shape[0] < 1 or dy.shape[1] < 1:
        raise ValueError(f"dy is {tuple(dy.shape)}: expected [M >= 1, N >= 1]")
    M, N = dy.shape
    on = _fused_state(adam, _lib.NdAdamStep, return_grad, "bias_grad_adam", dy.device, ((bias, "bias", (N,)), (m, "m", (N,)), (v, "v", (N,))))
    g = torch.empty(N, dtype=torch.float32, device=dy.device) if return_grad else None
    check(_lib.load().nd_bias_grad_adam(ptr(dy), ptr(bias) if on else None, ptr(m) if on else None, ptr(v) if on else None, ptr(g), M, N,
                                        float(gscale), ctypes.byref(adam) if on else None, _stream(dy)), "nd_bias_grad_adam")
    return g


COLSUM_CHUNK = 64                                          # ND_COLSUM_CHUNK: rows per partial of the column sums


def gemm_tn_adamw(dy: torch.Tensor, x: torch.Tensor, w: Optional[torch.Tensor], m: Optional[torch.Tensor], v: Optional[torch.Tensor], adamw,
                  gscale: float = 1.0, return_grad: bool = False) -> Optional[torch.Tensor]:
    """One AdamW step of a row-major fp32 weight w [N, K] on the gradient gscale * (dy^T @ x), dy [M, N], x [M, K], any M >= 1
    (nd_gemm_tn_adamw: the gradient is formed tile by tile and applied in registers, never written unless asked for).  w, m, v are
    updated IN PLACE.  adamw: ops.adamw_step(lr, t), or None for the gradient-only call (w, m, v unused).  return_grad: also return the
    gradient [N, K]."""
    dy, x = _f32(dy, "dy"), _f32(x, "x")
    if dy.dim() != 2 or x.dim() != 2 or dy.shape[0] < 1 or dy.shape[1] < 1 or x.shape[0] != dy.shape[0] or x.device != dy.device:
        raise ValueError(f"dy is {tuple(dy.shape)} on {dy.device}, x is {tuple(x.shape)} on {x.device}: expected [M >= 1, N >= 1] and [M, K]")
    (M, N), K = dy.shape, x.shape[1]
    if K < 16 or K % 16:
        raise ValueError(f"K must be a positive multiple of 16 (K={K})")
    on = _fused_state(adamw, _lib.NdAdamwStep, return_grad, "gemm_tn_adamw", dy.device, ((w, "w", N * K), (m, "m", N * K), (v, "v", N * K)))
    g = torch.empty(N, K, dtype=torch.float32, device=dy.device) if return_grad else None
    check(_lib.load().nd_gemm_tn_adamw(ptr(dy), ptr(x), ptr(w) if on else None, ptr(m) if on else None, ptr(v) if on else None, ptr(g), M, N, K,
                                       float(gscale), ctypes.byref(adamw) if on else None, _stream(dy)), "nd_gemm_tn_adamw")
    return g


def gemm_tn_plan(N: int, K: int) -> dict:
    """The tile geometry of nd_gemm_tn_adamw for an [N, K] result (host only)."""
    out = (ctypes.c_int * 5)()
    check(_lib.load().nd_gemm_tn_plan(int(N), int(K), out), "nd_gemm_tn_plan")
    return {"tile_n": out[0], "tile_k": out[1], "m_tile": out[2], "grid_k": out[3], "grid_n": out[4]}


def colsum_adamw(dy: torch.Tensor, b: Optional[torch.Tensor], m: Optional[torch.Tensor], v: Optional[torch.Tensor], adamw,
                 gscale: float = 1.0, return_grad: bool = False) -> Optional[torch.Tensor]:
    """One AdamW step of a vector parameter b (N elements, any shape) on the gradient gscale * dy.sum(0), dy [M, N], in place
    (nd_colsum_adamw).  The sum runs over chunks of COLSUM_CHUNK rows, each in row order, the partials in chunk order.  adamw None: the
    gradient-only call, returns [N]."""
    dy = _f32(dy, "dy")
    if dy.dim() != 2 or dy.shape[0] < 1 or dy.shape[1] < 1:
        raise ValueError(f"dy is {tuple(dy.shape)}: expected [M >= 1, N >= 1]")
    M, N = dy.shape
    on = _fused_state(adamw, _lib.NdAdamwStep, return_grad, "colsum_adamw", dy.device, ((b, "b", N), (m, "m", N), (v, "v", N)))
    g = torch.empty(N, dtype=torch.float32, device=dy.device) if return_grad else None
    check(_lib.load().nd_colsum_adamw(ptr(dy), ptr(b) if on else None, ptr(m) if on else None, ptr(v) if on else None, ptr(g), M, N,
                                      float(gscale), ctypes.byref(adamw) if on else None, _stream(dy)), "nd_colsum_adamw")
    return g


def layernorm_wgrad_adamw(x: torch.Tensor, g: torch.Tensor, eps: float, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor],
                          m_gamma: Optional[torch.Tensor], v_gamma: Optional[torch.Tensor], m_beta: Optional[torch.Tensor],
                          v_beta: Optional[torch.Tensor], adamw, gscale: float = 1.0, return_grad: bool = False):
    """One AdamW step of LayerNorm's gamma and beta [dim] on gscale * (sum_r g * xhat, sum_r g), x the LayerNorm's input [rows, dim], g =
    dL/d(its output), in place (nd_layernorm_wgrad_adamw; xhat recomputed from x as nd_layernorm does).  adamw None: the gradient-only
    call, returns (dgamma, dbeta)."""
    x, g = _f32(x, "x"), _f32(g, "g")
    if x.dim() != 2 or g.shape != x.shape or g.device != x.device or x.shape[0] < 1:
        raise ValueError(f"x is {tuple(x.shape)}, g is {tuple(g.shape)}: expected two [rows >= 1, dim] tensors on one device")
    rows, dim = x.shape
    if dim < 4 or dim % 4 or dim > 2048:
        raise ValueError(f"dim must be a multiple of 4 in [4, 2048] (dim={dim})")
    names = ("gamma", "beta", "m_gamma", "v_gamma", "m_beta", "v_beta")
    on = _fused_state(adamw, _lib.NdAdamwStep, return_grad, "layernorm_wgrad_adamw", x.device,
                      [(t, n, dim) for t, n in zip((gamma, beta, m_gamma, v_gamma, m_beta, v_beta), names)])
    dg = torch.empty(dim, dtype=torch.float32, device=x.device) if return_grad else None
    db = torch.empty(dim, dtype=torch.float32, device=x.device) if return_grad else None
    p = [ptr(t) if on else None for t in (gamma, beta, m_gamma, v_gamma, m_beta, v_beta)]
    lib = _lib.load()
    ws = _workspace(lib.nd_layernorm_wgrad_workspace_bytes(rows, dim), x.device)      # the per-chunk partials
    check(lib.nd_layernorm_wgrad_adamw(ptr(x), ptr(g), *p, ptr(dg), ptr(db), rows, dim, float(eps), float(gscale),
                                       ctypes.byref(adamw) if on else None, ptr(ws), ws.numel(), _stream(x)), "nd_layernorm_wgrad_adamw")
    return (dg, db) if return_grad else None
