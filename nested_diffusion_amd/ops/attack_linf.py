"""The Linf attack steps (FGSM / PGD) and AutoAttack's APGD-CE.  Binds csrc/nd_attack_linf.hip (include/nested_diffusion.h: nd_linf_* of
"input gradient of the full ViT and the Linf attacks", and "AutoAttack's APGD-CE, Linf"; the loops: attack.py, autoattack.py)."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib
from .._lib import check, ptr
from ._base import _DeviceState, _f32, _index, _inplace, _labels, _per_image, _stream, _u32, _u64


def linf_step(x: torch.Tensor, x0: torch.Tensor, grad: Optional[torch.Tensor], alpha: float, eps: float, lo: float = 0.0,
              hi: float = 1.0) -> torch.Tensor:
    """clip(x0 + clip(x + alpha * sign(grad) - x0, -eps, eps), lo, hi) (foolbox's step, project, clip).  grad None: no step --
    with lo = -inf, hi = inf that is foolbox's final clip_perturbation."""
    x, x0 = _f32(x, "x"), _f32(x0, "x0")
    if x0.shape != x.shape:
        raise ValueError("x0 must have the shape of x")
    if grad is not None:
        grad = _f32(grad, "grad")
        if grad.shape != x.shape:
            raise ValueError("grad must have the shape of x")
    out = torch.empty_like(x)
    check(_lib.load().nd_linf_step(ptr(x), ptr(x0), ptr(grad), ptr(out), x.numel(), float(alpha), float(eps), float(lo), float(hi),
                                   _stream(x)), "nd_linf_step")
    return out


def linf_random_start(x0: torch.Tensor, eps: float, seed: int, first_image: int = 0, restart: int = 0, lo: float = 0.0,
                      hi: float = 1.0) -> torch.Tensor:
    """clip(x0 + U[-eps, eps), lo, hi) per image; the draws of image b are keyed on (seed, first_image + b, element, restart), so an
    image draws the same start at any batch size (include/nested_diffusion.h: nd_linf_random_start)."""
    x0 = _f32(x0, "x0")
    B = x0.shape[0]
    per = x0.numel() // max(B, 1)                          # not _per_image: an empty batch is accepted here
    if per % 4:
        raise ValueError("the elements per image must be a multiple of 4")
    out = torch.empty_like(x0)
    check(_lib.load().nd_linf_random_start(ptr(x0), ptr(out), B, per, _u64(seed), _u32(first_image), _u32(restart), float(eps), float(lo),
                                           float(hi), _stream(x0)), "nd_linf_random_start")
    return out


APGD_NOT_PRED, APGD_IMPROVED, APGD_RESTORE = 1, 2, 4       # ND_APGD_* flag bits


def apgd_random_start(x0: torch.Tensor, index: torch.Tensor, eps: float, seed: int, restart: int = 0, lo: float = 0.0,
                      hi: float = 1.0) -> torch.Tensor:
    """APGD's start clip(x0 + eps * t / (max|t| + 1e-12), lo, hi), t = 2 U[0, 1) - 1 per element, max per image; row b draws with the key
    (seed, index[b], element, restart), so a row of a compacted subset draws what it draws in the full batch."""
    x0 = _f32(x0, "x0")
    B, per = _per_image(x0)
    index = _index(index, B, x0.device)
    out = torch.empty_like(x0)
    m_ws = torch.empty(B, dtype=torch.int32, device=x0.device)
    check(_lib.load().nd_apgd_random_start(ptr(x0), ptr(index), ptr(out), ptr(m_ws), B, per, _u64(seed), _u32(restart), float(eps), float(lo),
                                           float(hi), _stream(x0)), "nd_apgd_random_start")
    return out


class ApgdState(_DeviceState):
    """APGD's per-image state on the device (nd_apgd_control): step, loss_best, loss_best_last_check (fp32 [B]), reduced_last_check, acc
    (int32 [B]), loss_steps (fp32 [n_iter, B]) and the flags of the last iteration (int32 [B])."""

    def __init__(self, B: int, n_iter: int, device):
        self.B, self.n_iter = B, n_iter
        f32, i32 = torch.float32, torch.int32
        self.fields = (("step", f32, (B,)), ("loss_best", f32, (B,)), ("loss_best_last_check", f32, (B,)), ("reduced_last_check", i32, (B,)),
                       ("acc", i32, (B,)), ("flags", i32, (B,)), ("loss_steps", f32, (n_iter, B)))
        for name, dtype, shape in self.fields:
            setattr(self, name, torch.empty(shape, dtype=dtype, device=device))


def apgd_control(logits: torch.Tensor, labels: torch.Tensor, loss: torch.Tensor, state: ApgdState, it: int, k: int = 0, rho: float = 0.75,
                 step0: float = 0.0) -> torch.Tensor:
    """APGD's per-image bookkeeping of iteration `it` (-1: initialise from the start point, step = step0), with a checkpoint of length k
    when k > 0; updates `state` in place on the device and returns state.flags (APGD_NOT_PRED | APGD_IMPROVED | APGD_RESTORE).
    Nothing is read back to the host."""
    logits = _f32(logits, "logits")
    if logits.dim() != 2:
        raise ValueError("logits must be [B, C]")
    B, C = logits.shape
    if C < 1 or C > 1024:
        raise ValueError(f"apgd control takes 1 <= C <= 1024 classes (C={C})")
    if B != state.B:
        raise ValueError(f"logits has {B} rows, the state {state.B}")
    loss = _f32(loss, "loss")
    labels = _labels(labels, logits.device, B, who="labels and loss", also=(loss,))
    if not -1 <= it < state.n_iter or not 0 <= k <= it + 1:
        raise ValueError(f"need -1 <= it < n_iter and 0 <= k <= it + 1 (it={it}, k={k}, n_iter={state.n_iter})")
    s = state
    s.check(B)
    check(_lib.load().nd_apgd_control(ptr(logits), ptr(labels), ptr(loss), ptr(s.step), ptr(s.loss_best), ptr(s.loss_best_last_check),
                                      ptr(s.reduced_last_check), ptr(s.acc), ptr(s.loss_steps), ptr(s.flags), B, C, s.n_iter, int(it),
                                      int(k), float(rho), float(step0), _stream(logits)), "nd_apgd_control")
    return s.flags


def apgd_update(x: torch.Tensor, x_adv: torch.Tensor, x_adv_old: Optional[torch.Tensor], grad: torch.Tensor,
                x_best: Optional[torch.Tensor], grad_best: Optional[torch.Tensor], x_best_adv: Optional[torch.Tensor],
                flags: Optional[torch.Tensor], step: Optional[torch.Tensor], eps: float, a: float, do_step: bool) -> None:
    """APGD's per-element work of one iteration, in place: the flags' copies (x_best_adv, x_best / grad_best, the restore), then with
    do_step the momentum step of coefficient a from x_adv (or the restored x_best) to the next iterate (x_adv, x_adv_old).
    flags None: the step alone (the first step: a = 1, with x_adv_old a copy of x_adv)."""
    x_adv = _inplace(x_adv, "x_adv")
    B, per = _per_image(x_adv)
    shape = tuple(x_adv.shape)
    grad = _inplace(grad, "grad", shape=shape)
    if flags is not None:
        flags = _inplace(flags, "flags", torch.int32, (B,))
        if x_best is None or grad_best is None or x_best_adv is None:
            raise ValueError("the flags need x_best, grad_best and x_best_adv")
        x_best, grad_best, x_best_adv = (_inplace(t, n, shape=shape) for t, n in ((x_best, "x_best"), (grad_best, "grad_best"),
                                                                                   (x_best_adv, "x_best_adv")))
    if do_step:
        if x is None or x_adv_old is None or step is None:
            raise ValueError("a step needs x, x_adv_old and step")
        x, x_adv_old = _inplace(x, "x", shape=shape), _inplace(x_adv_old, "x_adv_old", shape=shape)
        step = _inplace(step, "step", shape=(B,))
    check(_lib.load().nd_apgd_update(ptr(x) if do_step else None, ptr(x_adv), ptr(x_adv_old) if do_step else None, ptr(grad),
                                     ptr(x_best), ptr(grad_best), ptr(x_best_adv), ptr(flags), ptr(step) if do_step else None, B, per,
                                     float(eps), float(a), int(bool(do_step)), _stream(x_adv)), "nd_apgd_update")
