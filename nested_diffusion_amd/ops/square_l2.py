"""The Square attack, L2: the start, the proposal and the commit of a query.  Binds csrc/nd_square_l2.hip (include/nested_diffusion.h:
"the Square attack, L2"; the loop: square.py of the package).  The accept step is square_accept of the Linf form."""
from __future__ import annotations

from typing import Tuple

import torch

from .. import _lib
from .._lib import check, ptr
from ._base import _f32, _image4, _index, _inplace, _stream, _u32, _u64
from .square import SquareState

SQUARE_L2_SUMS = 6                                         # ND_SQUARE_L2_SUMS: S_w1, S_all, S_mask, S_out, S_u, S_new
SQUARE_L2_MIN_DIM = 5


def square_l2_ws_floats(Cin: int, H: int, W: int) -> int:
    """Floats of workspace per image (the partials of the row sums)."""
    n = int(_lib.load().nd_square_l2_ws_floats(int(Cin), int(H), int(W)))
    if n == 0:
        raise ValueError(f"square L2 takes 1 <= Cin <= 32 and 5 <= H, W <= 4096 (Cin={Cin}, H={H}, W={W})")
    return n


class SquareL2State(SquareState):
    """SquareState's fields with the two window corners of the last proposal (win, int32 [B, 4]: vh1, vw1, vh2, vw2), the six sums it
    used (sums, fp32 [6, B]) and the workspace of the row sums for images of Cin x H x W."""

    def __init__(self, B: int, Cin: int, H: int, W: int, device):
        super().__init__(B, device)
        self.fields = tuple(f for f in self.fields if f[0] != "win") + (("win", torch.int32, (B, 4)), ("sums", torch.float32, (SQUARE_L2_SUMS, B)),
                                                                         ("ws", torch.float32, (B * square_l2_ws_floats(Cin, H, W),)))
        self.win = torch.zeros((B, 4), dtype=torch.int32, device=device)
        self.sums = torch.zeros((SQUARE_L2_SUMS, B), dtype=torch.float32, device=device)
        self.ws = torch.empty(self.fields[-1][2], dtype=torch.float32, device=device)       # written before it is read


def _eta(eta: torch.Tensor, s: int, device) -> torch.Tensor:
    if tuple(eta.shape) != (s, s) or eta.device != device:
        raise ValueError(f"eta is {tuple(eta.shape)} on {eta.device}; expected [{s}, {s}] on {device}")
    return _f32(eta, "eta")


def square_l2_init(x0: torch.Tensor, index: torch.Tensor, eta0: torch.Tensor, eps: float, seed: int, restart: int = 0, lo: float = 0.0,
                   hi: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(x_best, x_new, sum D0^2 [B]): both arrays the start clip(x0 + D0 / (1e-12 + ||D0||) * eps, lo, hi), D0 the tiling of the image by
    +-eta(s0) or its transpose, s0 = min(H, W) // 5; row b draws with the key (seed, index[b], tile, restart)."""
    x0 = _f32(x0, "x0")
    B, Cin, H, W = _image4(x0, "x0")
    if min(H, W) < SQUARE_L2_MIN_DIM:
        raise ValueError(f"square L2 needs images of at least 5 x 5 (H={H}, W={W})")
    s0 = min(H, W) // 5
    index = _index(index, B, x0.device)
    eta0 = _eta(eta0, s0, x0.device)
    x_best, x_new = torch.empty_like(x0), torch.empty_like(x0)
    sums = torch.empty(B, dtype=torch.float32, device=x0.device)
    ws = torch.empty(B * square_l2_ws_floats(Cin, H, W), dtype=torch.float32, device=x0.device)
    check(_lib.load().nd_square_l2_init(ptr(x0), ptr(index), ptr(eta0), ptr(x_best), ptr(x_new), ptr(sums), ptr(ws), B, Cin, H, W, s0, _u64(seed),
                                        _u32(restart), float(eps), float(lo), float(hi), _stream(x0)), "nd_square_l2_init")
    return x_best, x_new, sums


def square_l2_propose(x0: torch.Tensor, x_best: torch.Tensor, x_new: torch.Tensor, index: torch.Tensor, state: SquareL2State,
                      eta: torch.Tensor, s: int, it: int, eps: float, seed: int, restart: int = 0, lo: float = 0.0, hi: float = 1.0) -> None:
    """Query `it` of the rows still active (state.margin_min > 0): draws each row's two windows, signs and transpose bit, moves the norm
    budget of window 2 into window 1 along +-eta(s) and rewrites the whole of x_new on the eps-sphere; the corners go to state.win and
    the six sums the passes used to state.sums.  In place; frozen rows are not touched."""
    x_new = _inplace(x_new, "x_new")
    B, Cin, H, W = _image4(x_new, "x_new")
    shape = tuple(x_new.shape)
    x0, x_best = _inplace(x0, "x0", shape=shape), _inplace(x_best, "x_best", shape=shape)
    index = _index(index, B, x_new.device)
    state.check(B)
    if not 3 <= s <= min(H, W) or s % 2 == 0 or it < 0:
        raise ValueError(f"need an odd s, 3 <= s <= min(H, W), and it >= 0 (s={s}, H={H}, W={W}, it={it})")
    eta = _eta(eta, s, x_new.device)
    check(_lib.load().nd_square_l2_propose(ptr(x0), ptr(x_best), ptr(x_new), ptr(index), ptr(state.margin_min), ptr(eta), ptr(state.win),
                                           ptr(state.sums), ptr(state.ws), B, Cin, H, W, int(s), int(it), _u64(seed), _u32(restart), float(eps),
                                           float(lo), float(hi), _stream(x_new)), "nd_square_l2_propose")


def square_l2_commit(x_best: torch.Tensor, x_new: torch.Tensor, state: SquareState) -> None:
    """Accepted rows (state.flags == SQUARE_ACTIVE | SQUARE_ACCEPT): x_best = x_new over the whole image.  Nothing else: a rejected
    candidate stays in x_new until the next propose rewrites it."""
    x_new = _inplace(x_new, "x_new")
    B, Cin, H, W = _image4(x_new, "x_new")
    x_best = _inplace(x_best, "x_best", shape=tuple(x_new.shape))
    state.check(B)
    check(_lib.load().nd_square_l2_commit(ptr(x_best), ptr(x_new), ptr(state.flags), B, Cin * H * W, _stream(x_new)), "nd_square_l2_commit")
