"""The L2 attacks (BIM, L2PGD) and Carlini & Wagner.  Binds csrc/nd_attack_l2.hip and nd_margin_head_bwd of csrc/nd_vit_grad.hip
(include/nested_diffusion.h: "the L2 attacks ... and Carlini & Wagner's L2 attack"; the loops: attack.py)."""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from .. import _lib
from .._lib import check, ptr
from ._base import _DeviceState, _f32, _inplace, _labels, _per_image, _stream, _u32, _u64

L2_MAX_PARTS = 256                                         # ND_L2_MAX_PARTS: partials per image of a row reduction


def _l2_ws(B: int, device, sums: int = 2) -> torch.Tensor:
    """The row reductions' workspace: ND_L2_MAX_PARTS partials per image and sum (written before it is read: no initialisation)."""
    return torch.empty(sums * L2_MAX_PARTS * B, dtype=torch.float32, device=device)


def margin_head_grad(logits: torch.Tensor, labels: torch.Tensor, consts: torch.Tensor, head_w: torch.Tensor, confidence: float = 0.0,
                     check_labels: bool = True) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dfeat [B, E], margin [B], other [B] int32): the gradient of sum_b consts[b] * max(0, margin[b]) with respect to the head's input,
    margin = logits[label] - logits[other] + confidence, other = the first maximal non-label column (nd_margin_head_bwd).
    check_labels=False skips the label-range check, which reads back (the kernel gives an out-of-range label a NaN margin and no
    gradient): a loop that checked its labels once stays free of host synchronisation."""
    logits, head_w, consts = _f32(logits, "logits"), _f32(head_w, "head_w"), _f32(consts, "consts")
    if logits.dim() != 2:
        raise ValueError("logits must be [B, C]")
    B, C = logits.shape
    if C < 2 or C > 1024:
        raise ValueError(f"the margin needs 2 <= C <= 1024 classes (C={C})")
    if head_w.dim() != 2 or head_w.shape[0] != C:
        raise ValueError(f"head_w is {tuple(head_w.shape)}, logits {tuple(logits.shape)}")
    labels = _labels(labels, logits.device, B, C if check_labels else None, who="labels and consts", also=(consts,))
    E = head_w.shape[1]
    dfeat = torch.empty(B, E, dtype=torch.float32, device=logits.device)
    margin = torch.empty(B, dtype=torch.float32, device=logits.device)
    other = torch.empty(B, dtype=torch.int32, device=logits.device)
    check(_lib.load().nd_margin_head_bwd(ptr(logits), ptr(labels), ptr(consts), ptr(head_w), ptr(dfeat), ptr(margin), ptr(other), B, C, E,
                                         float(confidence), _stream(logits)), "nd_margin_head_bwd")
    return dfeat, margin, other


def l2_step(x: torch.Tensor, x0: torch.Tensor, grad: Optional[torch.Tensor], alpha: float, eps: float, lo: float = 0.0, hi: float = 1.0,
            want_norms: bool = False):
    """foolbox's L2 step, project, clip per image: t = x + alpha * g / max(||g||, 1e-12), d = t - x0,
    clip(x0 + d * min(1, eps / max(||d||, 1e-12)), lo, hi).  grad None: no step -- with lo = -inf, hi = inf that is the final
    clip_perturbation.  want_norms: also (gnorm, dnorm) [B], the values the elementwise pass used (gnorm 0 without a gradient)."""
    x, x0 = _f32(x, "x"), _f32(x0, "x0")
    if x0.shape != x.shape:
        raise ValueError("x0 must have the shape of x")
    B, per = _per_image(x)
    if grad is not None:
        grad = _f32(grad, "grad")
        if grad.shape != x.shape:
            raise ValueError("grad must have the shape of x")
    out = torch.empty_like(x)
    gnorm = torch.empty(B, dtype=torch.float32, device=x.device)
    dnorm = torch.empty(B, dtype=torch.float32, device=x.device)
    check(_lib.load().nd_l2_step(ptr(x), ptr(x0), ptr(grad), ptr(out), ptr(gnorm), ptr(dnorm), ptr(_l2_ws(B, x.device)), B, per, float(alpha),
                                 float(eps), float(lo), float(hi), _stream(x)), "nd_l2_step")
    return (out, gnorm, dnorm) if want_norms else out


def l2_random_start(x0: torch.Tensor, eps: float, seed: int, first_image: int = 0, restart: int = 0, lo: float = 0.0, hi: float = 1.0,
                    want_norm: bool = False):
    """clip(x0 + eps * r, lo, hi), r uniform in the unit n-ball (foolbox's uniform_n_balls: the first n of n + 2 normals over the norm of
    all n + 2); the normals of image b are keyed on (seed, first_image + b, element, restart).  want_norm: also snorm [B]."""
    x0 = _f32(x0, "x0")
    B, per = _per_image(x0)
    out = torch.empty_like(x0)
    snorm = torch.empty(B, dtype=torch.float32, device=x0.device)
    check(_lib.load().nd_l2_random_start(ptr(x0), ptr(out), ptr(snorm), ptr(_l2_ws(B, x0.device, 1)), B, per, _u64(seed), _u32(first_image),
                                         _u32(restart), float(eps), float(lo), float(hi), _stream(x0)), "nd_l2_random_start")
    return (out, snorm) if want_norm else out


def cw_attack_space(x0: torch.Tensor, lo: float = 0.0, hi: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(w0, xrec): w0 = atanh(((x0 - a) / b) * 0.999999), xrec = tanh(w0) * b + a, a = (lo + hi) / 2, b = (hi - lo) / 2."""
    x0 = _f32(x0, "x0")
    if x0.numel() == 0 or x0.numel() % 4:
        raise ValueError("the number of elements must be a positive multiple of 4")
    w0, xrec = torch.empty_like(x0), torch.empty_like(x0)
    check(_lib.load().nd_cw_attack_space(ptr(x0), ptr(w0), ptr(xrec), x0.numel(), float(lo), float(hi), _stream(x0)), "nd_cw_attack_space")
    return w0, xrec


class CwState(_DeviceState):
    """Carlini & Wagner's device state for B images shaped like x0: the tanh-space variable delta with Adam's m and v, the iterate's t and x,
    best / best_norm over all binary-search steps, and the per-image scalars of an iteration (sq_rec, sq_x0, found, flags, loss)."""

    def __init__(self, x0: torch.Tensor):
        x0 = _f32(x0, "x0")
        self.B, self.per = _per_image(x0)
        dev, B = x0.device, self.B
        self.delta, self.m, self.v = torch.zeros_like(x0), torch.zeros_like(x0), torch.zeros_like(x0)
        self.t, self.x = torch.empty_like(x0), torch.empty_like(x0)
        self.best = torch.zeros_like(x0)
        self.best_norm = torch.full((B,), float("inf"), dtype=torch.float32, device=dev)
        self.sq_rec, self.sq_x0, self.loss = (torch.empty(B, dtype=torch.float32, device=dev) for _ in range(3))
        self.found, self.flags = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        self.ws = _l2_ws(B, dev)
        f32, i32 = torch.float32, torch.int32                # what nd_cw_control takes
        self.fields = (("sq_rec", f32, (B,)), ("sq_x0", f32, (B,)), ("best_norm", f32, (B,)), ("loss", f32, (B,)), ("found", i32, (B,)),
                       ("flags", i32, (B,)))

    def reset_search_step(self) -> None:
        """The start of a binary-search step: delta = 0, Adam's state = 0, found = False (best and best_norm carry over)."""
        for t in (self.delta, self.m, self.v, self.found):
            t.zero_()


def cw_model_space(w0: torch.Tensor, x0: torch.Tensor, xrec: torch.Tensor, s: CwState, lo: float = 0.0, hi: float = 1.0) -> torch.Tensor:
    """s.t = tanh(w0 + s.delta), s.x = s.t * b + a, s.sq_rec = sum (x - xrec)^2, s.sq_x0 = sum (x - x0)^2 per image; returns s.x."""
    shape = tuple(s.delta.shape)
    w0, x0, xrec = (_inplace(t, n, shape=shape) for t, n in ((w0, "w0"), (x0, "x0"), (xrec, "xrec")))
    check(_lib.load().nd_cw_model_space(ptr(w0), ptr(s.delta), ptr(x0), ptr(xrec), ptr(s.t), ptr(s.x), ptr(s.sq_rec), ptr(s.sq_x0), ptr(s.ws),
                                        s.B, s.per, float(lo), float(hi), _stream(w0)), "nd_cw_model_space")
    return s.x


def cw_control(logits: torch.Tensor, labels: torch.Tensor, consts: torch.Tensor, margin: torch.Tensor, s: CwState,
               confidence: float = 0.0) -> torch.Tensor:
    """The per-image bookkeeping of one CW iteration (nd_cw_control), in place on s: found |= adv, best_norm, flags = new best,
    loss = consts * max(0, margin) + sq_rec.  Nothing is read back; returns s.loss."""
    logits = _f32(logits, "logits")
    if logits.dim() != 2 or logits.shape[0] != s.B:
        raise ValueError(f"logits must be [{s.B}, C]")
    B, C = logits.shape
    if C < 2 or C > 1024:
        raise ValueError(f"cw control takes 2 <= C <= 1024 classes (C={C})")
    consts, margin = _f32(consts, "consts"), _f32(margin, "margin")
    labels = _labels(labels, logits.device, B, who="labels, consts and margin", also=(consts, margin))
    s.check(B)
    check(_lib.load().nd_cw_control(ptr(logits), ptr(labels), ptr(consts), ptr(margin), ptr(s.sq_rec), ptr(s.sq_x0), ptr(s.best_norm),
                                    ptr(s.found), ptr(s.flags), ptr(s.loss), B, C, float(confidence), _stream(logits)), "nd_cw_control")
    return s.loss


def cw_b_half(lo: float, hi: float) -> float:
    """b = (hi - lo) / 2 as nd_cw_attack_space and nd_cw_model_space form it: float32 lo and hi, float32 arithmetic (each double operation
    on float32 operands, rounded to float32, is the float32 operation).  nd_cw_update's b_half must be this value, not the double's rounding:
    at (-0.3, 1.1) the two differ by an ulp."""
    r = lambda v: ctypes.c_float(v).value                                  # noqa: E731
    return r(r(r(hi) - r(lo)) / 2.0)


def cw_update(s: CwState, dx: torch.Tensor, xrec: torch.Tensor, stepsize: float, k: int, lo: float = 0.0, hi: float = 1.0,
              use_flags: bool = True) -> None:
    """Iteration k's per-element pass (nd_cw_update), in place on s: best = x in the flagged rows, then the tanh-space gradient of
    sum_b loss_b from dx and the Adam update of delta with the bias corrections of step k + 1 (computed here in double).  dx is
    taken as it is: a non-contiguous one is refused, not copied."""
    shape = tuple(s.delta.shape)
    dx, xrec = _inplace(dx, "dx", shape=shape), _inplace(xrec, "xrec", shape=shape)
    bc1, bc2 = 1.0 - 0.9 ** (k + 1), 1.0 - 0.999 ** (k + 1)
    check(_lib.load().nd_cw_update(ptr(s.delta), ptr(s.m), ptr(s.v), ptr(dx), ptr(s.x), ptr(xrec), ptr(s.t), ptr(s.best),
                                   ptr(s.flags) if use_flags else None, s.B, s.per, float(stepsize), bc1, bc2, cw_b_half(lo, hi),
                                   _stream(dx)), "nd_cw_update")
