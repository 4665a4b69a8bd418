"""The Square attack, Linf: the three launches of a query.  Binds csrc/nd_square.hip (include/nested_diffusion.h: "the Square attack,
Linf"; the loop: square.py of the package)."""
from __future__ import annotations

from typing import Tuple

import torch

from .. import _lib
from .._lib import check, ptr
from ._base import _DeviceState, _f32, _image4, _index, _inplace, _labels, _stream, _u32, _u64

SQUARE_ACTIVE, SQUARE_ACCEPT = 1, 2                        # ND_SQUARE_* flag bits


class SquareState(_DeviceState):
    """The Square attack's per-image state on the device (nd_square_accept): margin_min, loss_min (fp32 [B]), n_queries and the flags of
    the last query (int32 [B]), and the window corner (vh, vw) of the last proposal (win, int32 [B, 2])."""

    def __init__(self, B: int, device):
        self.B = B
        self.fields = (("margin_min", torch.float32, (B,)), ("loss_min", torch.float32, (B,)), ("n_queries", torch.int32, (B,)),
                       ("flags", torch.int32, (B,)), ("win", torch.int32, (B, 2)))
        for name, dtype, shape in self.fields:
            setattr(self, name, torch.empty(shape, dtype=dtype, device=device))
        self.win.zero_()


def square_init(x0: torch.Tensor, index: torch.Tensor, eps: float, seed: int, restart: int = 0, lo: float = 0.0,
                hi: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(x_best, x_new), both the vertical-stripe start clip(x0 + eps * sigma(b, c, w), lo, hi); row b draws its signs with the key
    (seed, index[b], c * W + w, restart), so a row of a compacted subset draws what it draws in the full batch."""
    x0 = _f32(x0, "x0")
    B, Cin, H, W = _image4(x0, "x0")
    index = _index(index, B, x0.device)
    x_best, x_new = torch.empty_like(x0), torch.empty_like(x0)
    check(_lib.load().nd_square_init(ptr(x0), ptr(index), ptr(x_best), ptr(x_new), B, Cin, H, W, _u64(seed), _u32(restart), float(eps),
                                     float(lo), float(hi), _stream(x0)), "nd_square_init")
    return x_best, x_new


def square_propose(x0: torch.Tensor, x_best: torch.Tensor, x_new: torch.Tensor, index: torch.Tensor, state: SquareState, s: int, it: int,
                   eps: float, seed: int, restart: int = 0, lo: float = 0.0, hi: float = 1.0) -> None:
    """Query `it` of the rows still active (state.margin_min > 0): draws each row's window and per-channel signs, writes the candidate
    clip(min(max(x_best +- 2 eps, x0 - eps), x0 + eps), lo, hi) into that window of x_new and the corner into state.win.  In place;
    frozen rows are not touched."""
    x_new = _inplace(x_new, "x_new")
    B, Cin, H, W = _image4(x_new, "x_new")
    shape = tuple(x_new.shape)
    x0, x_best = _inplace(x0, "x0", shape=shape), _inplace(x_best, "x_best", shape=shape)
    index = _index(index, B, x_new.device)
    state.check(B)
    if not 1 <= s <= min(H, W) or it < 0:
        raise ValueError(f"need 1 <= s <= min(H, W) and it >= 0 (s={s}, H={H}, W={W}, it={it})")
    check(_lib.load().nd_square_propose(ptr(x0), ptr(x_best), ptr(x_new), ptr(index), ptr(state.margin_min), ptr(state.win), B, Cin, H, W,
                                        int(s), int(it), _u64(seed), _u32(restart), float(eps), float(lo), float(hi), _stream(x_new)),
          "nd_square_propose")


def square_accept(scores: torch.Tensor, labels: torch.Tensor, state: SquareState, it: int) -> torch.Tensor:
    """The bookkeeping of query `it` (-1: initialise from the start point's scores) on the device: the margin of each row, the accept rule,
    the query count; updates `state` in place and returns state.flags (SQUARE_ACTIVE | SQUARE_ACCEPT).  Nothing is read back."""
    scores = _f32(scores, "scores")
    if scores.dim() != 2:
        raise ValueError("scores must be [B, C]")
    B, C = scores.shape
    if C < 2 or C > 1024:
        raise ValueError(f"square accept takes 2 <= C <= 1024 classes (C={C})")
    labels = _labels(labels, scores.device, B)
    state.check(B)
    if it < -1:
        raise ValueError(f"need it >= -1 (it={it})")
    check(_lib.load().nd_square_accept(ptr(scores), ptr(labels), ptr(state.margin_min), ptr(state.loss_min), ptr(state.n_queries),
                                       ptr(state.flags), B, C, int(it), _stream(scores)), "nd_square_accept")
    return state.flags


def square_commit(x_best: torch.Tensor, x_new: torch.Tensor, state: SquareState, s: int) -> None:
    """Over each active row's window (state.win, side s of the propose): an accepted candidate becomes x_best, a rejected one is
    restored from x_best.  Afterwards x_new == x_best everywhere."""
    x_new = _inplace(x_new, "x_new")
    B, Cin, H, W = _image4(x_new, "x_new")
    x_best = _inplace(x_best, "x_best", shape=tuple(x_new.shape))
    state.check(B)
    if not 1 <= s <= min(H, W):
        raise ValueError(f"need 1 <= s <= min(H, W) (s={s}, H={H}, W={W})")
    check(_lib.load().nd_square_commit(ptr(x_best), ptr(x_new), ptr(state.win), ptr(state.flags), B, Cin, H, W, int(s), _stream(x_new)),
          "nd_square_commit")
