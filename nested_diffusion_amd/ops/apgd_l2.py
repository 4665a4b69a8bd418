"""AutoAttack's APGD with norm = 'L2' and the accumulation of an expectation over transformation.  Binds csrc/nd_apgd_l2.hip
(include/nested_diffusion.h: "AutoAttack's APGD, L2"; the loops: autoattack.py, eot.py)."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib
from .._lib import check, ptr
from ._base import _f32, _index, _inplace, _per_image, _stream, _u32, _u64
from .attack_l2 import _l2_ws


def apgd_l2_random_start(x0: torch.Tensor, index: torch.Tensor, eps: float, seed: int, restart: int = 0, lo: float = 0.0, hi: float = 1.0,
                         want_norm: bool = False):
    """APGD's L2 start clip(x0 + eps * t / (||t|| + 1e-12), lo, hi), t per_image standard normals per image; row b draws with the key
    (seed, index[b], element, restart), so a row of a compacted subset draws what it draws in the full batch.  want_norm: also
    tnorm [B], the value the elementwise pass used."""
    x0 = _f32(x0, "x0")
    B, per = _per_image(x0)
    index = _index(index, B, x0.device)
    out = torch.empty_like(x0)
    tnorm = torch.empty(B, dtype=torch.float32, device=x0.device)
    check(_lib.load().nd_apgd_l2_random_start(ptr(x0), ptr(index), ptr(out), ptr(tnorm), ptr(_l2_ws(B, x0.device)), B, per, _u64(seed),
                                              _u32(restart), float(eps), float(lo), float(hi), _stream(x0)), "nd_apgd_l2_random_start")
    return (out, tnorm) if want_norm else out


def apgd_l2_step(x: torch.Tensor, x_adv: torch.Tensor, x_adv_old: torch.Tensor, grad: torch.Tensor, grad_best: Optional[torch.Tensor],
                 flags: Optional[torch.Tensor], step: torch.Tensor, eps: float, a: float) -> torch.Tensor:
    """APGD's L2 momentum step of coefficient a, in place on x_adv and x_adv_old (the listing: nd_apgd_l2_step in the header).  A row
    whose flags carry APGD_RESTORE steps along grad_best; flags None: every row along grad (the first step: a = 1, with x_adv_old a copy of
    x_adv).  Runs after apgd_update(..., do_step=False), which makes the flags' copies and the restore.  Returns norms [3, B]: the
    per-image ||g||, ||d1|| and ||d2|| the elementwise passes used."""
    x_adv = _inplace(x_adv, "x_adv")
    B, per = _per_image(x_adv)
    shape = tuple(x_adv.shape)
    x, x_adv_old, grad = (_inplace(t, n, shape=shape) for t, n in ((x, "x"), (x_adv_old, "x_adv_old"), (grad, "grad")))
    if flags is not None:
        flags = _inplace(flags, "flags", torch.int32, (B,))
        if grad_best is None:
            raise ValueError("the flags need grad_best")
        grad_best = _inplace(grad_best, "grad_best", shape=shape)
    step = _inplace(step, "step", shape=(B,))
    norms = torch.empty(3, B, dtype=torch.float32, device=x_adv.device)
    check(_lib.load().nd_apgd_l2_step(ptr(x), ptr(x_adv), ptr(x_adv_old), ptr(grad), ptr(grad_best) if flags is not None else None,
                                      ptr(flags), ptr(step), ptr(norms), ptr(_l2_ws(B, x_adv.device)), B, per, float(eps), float(a),
                                      _stream(x_adv)), "nd_apgd_l2_step")
    return norms


def eot_add(acc: torch.Tensor, g: torch.Tensor, divisor: int = 0) -> torch.Tensor:
    """acc += g in place; with divisor > 0, acc = (acc + g) / divisor (the last draw of a mean: one add and one true division per
    element).  Returns acc."""
    acc = _inplace(acc, "acc")
    g = _inplace(g, "g", shape=tuple(acc.shape))
    if acc.numel() % 4:
        raise ValueError("the number of elements must be a multiple of 4")
    if int(divisor) != divisor or divisor < 0:
        raise ValueError(f"divisor must be a non-negative integer (divisor={divisor})")
    check(_lib.load().nd_eot_add(ptr(acc), ptr(g), acc.numel(), int(divisor), _stream(acc)), "nd_eot_add")
    return acc
