"""Square attack (Linf) on the GPU: the score-based, black-box member of AutoAttack (Andriushchenko et al., ECCV 2020), with the
constructor and surface of autoattack's SquareAttack (square.py of autoattack 0.1).  It needs forward scores only, so it can be pointed at
anything that returns [B, C] scores, not only at the ViT the gradient attacks are aimed at.

autoattack is not a dependency here (it is not installed, as foolbox is not): the attack is restated on the library's kernels
(nd_square_init, nd_square_propose, nd_square_accept, nd_square_commit).  Parity is unpinned.  What is restated, from autoattack's
published square.py, Linf branch (all arrays per image; every operation one rounded fp32 op in this order):

    SquareAttack(predict, norm='Linf', n_queries=5000, eps=None, p_init=.8, n_restarts=1, seed=0, verbose=False, targeted=False,
                 loss='margin', resc_schedule=True, device=None)
    p_selection(it):  if resc_schedule: it = int(it / n_queries * 10000)
        p = p_init / 2^k for it in (10, 50], (50, 200], (200, 500], (500, 1000], (1000, 2000], (2000, 4000], (4000, 6000], (6000, 8000],
        (8000, inf), k = 1 .. 9; else p = p_init
    side(it, H, W) = min(max(int(round(sqrt(p_selection(it) * H * W))), 1), H, W)      (round is Python's)
    margin_and_loss(scores, y):  margin = scores[y] - max_{j != y} scores[j];  loss = margin             (untargeted, loss='margin')
    perturb(x, y):  acc = argmax(predict(x)) == y, adv = x; for r < n_restarts: run attack_single_run on the rows with acc still set;
        the rows argmax(predict(x_best)) misclassifies get acc = 0 and adv = x_best; every other row comes back unchanged
    attack_single_run(x, y):
        x_best = clamp(x + eps * sigma, 0, 1), sigma = +-1 per (image, channel, column): vertical stripes            nd_square_init
        margin_min, loss_min = margin_and_loss(predict(x_best), y);  n_queries = 1                            nd_square_accept, iter -1
        for i < n_queries, on the rows with margin_min > 0:
            s = side(i, H, W);  vh in [0, H - s], vw in [0, W - s];  d_c = +-2 eps per channel                       nd_square_propose
            x_new = x_best;  x_new[:, :, vh:vh+s, vw:vw+s] = clamp(min(max(x_best + d_c, x - eps), x + eps), 0, 1) over the window
            margin, loss = margin_and_loss(predict(x_new), y)                                                        nd_square_accept
            improved = loss < loss_min;  loss_min[improved] = loss
            accept = improved or margin <= 0;  margin_min[accept] = margin;  x_best[accept] = x_new[accept]          nd_square_commit
            n_queries += 1
        return n_queries, x_best

How the loop is laid out here: x_new is not a copy made per query.  It is a second array that equals x_best on every element after every
commit; a proposal writes the candidate into one window of it, the model reads it, and the commit either copies that window into x_best
(accept) or takes it back from x_best (reject).  The attack side of a query therefore moves Cin * s * s elements per image instead of
several passes over Cin * H * W.  A query is propose, predict, accept, commit; nothing is read back to the host except, every
check_every queries, one integer: the number of rows with margin_min > 0, at which the loop stops when it is zero.

Deviations, documented:
  - autoattack draws one window and one sign per channel for the whole batch, from torch.rand seeded with the clock.  Here every image draws
    its own window and signs from the library's Philox keyed on (seed, the image's global index, query, restart): the same image sees the
    same sequence of proposals in any batch, subset or rank.
  - autoattack compacts the batch to the rows not yet fooled at every query.  Here the batch keeps its shape and those rows are frozen:
    propose, accept and commit leave them alone (the model still evaluates them; their scores are ignored).
  - sigma and d_c are taken from one random bit each, where autoattack takes sign(2u - 1) of a uniform draw.
  - autoattack sets the window to x +- eps; here it is x_best +- 2 eps projected onto [x - eps, x + eps], which is the same point wherever
    x_best sits on the eps-sphere and cannot leave the ball where clipping to [0, 1] moved it off the sphere.
  - min(..., H, W) in side() is this project's clamp for images that are not square: the window has to fit both ways.  s is one host
    integer per query, shared by the batch.
  - a row whose scores contain a NaN has a NaN margin: it is never accepted and never counts as fooled inside attack_single_run, whereas the
    rows perturb selects on the host use torch.argmax, where a NaN wins.  The two differ only for a model that returns NaN scores.

predict is a VisionTransformer, a GuidingConditioner (its ViT, as for the other attacks) or any callable that maps a float32
[B, Cin, H, W] device tensor to a float32 [B, C] device tensor.

The L2 form (SquareL2Attack; nd_square_l2_init, nd_square_l2_propose, nd_square_accept, nd_square_l2_commit).  It is not the Linf kernels
with another constant: every query moves norm budget from one window to another and renormalises the whole perturbation to the
eps-sphere, so it needs per-image sums over masked regions and a whole-image rewrite per query.  Restated from autoattack's square.py,
L2 branch; this listing governs (all arrays per image; every elementwise operation one rounded fp32 op in this order; sums are fp32 in
an order fixed by (Cin, H, W, s, the windows), never by B or the row's place in the batch):

    eta_rectangles(a, b): d = zeros[a, b]; xc, yc = a//2 + 1, b//2 + 1; c2 = [xc - 1, yc - 1]
        for k in range(max(xc, yc)):
            d[max(c2[0],0):min(c2[0] + 2k + 1, a), max(c2[1],0):min(c2[1] + 2k + 1, b)] += 1/(k + 1)^2
            c2[0] -= 1; c2[1] -= 1
        return d / sqrt(sum d^2)
    eta(s): d = zeros[s, s]; d[:s//2] = eta_rectangles(s//2, s); d[s//2:] = -eta_rectangles(s - s//2, s)
        return d / sqrt(sum d^2)
            # host, float64, rounded once to fp32, cached per s, uploaded as [s, s]
            # eta(3) = [[.13608276, .68041382, .13608276],
            #           [-.12909944, -.12909944, -.12909944],
            #           [-.12909944, -.64549722, -.12909944]]
            # eta(1) = [[-1]]
    side_l2(it, H, W): s = max(int(round(sqrt(p_selection(it) * H * W))), 3)
        if s even: s += 1
        s = min(s, largest odd <= min(H, W))        # the min is this project's clamp
    init: s0 = min(H, W) // 5; nh, nw = H // s0, W // s0; oh, ow = (H - nh*s0)//2, (W - nw*s0)//2
        D0 = 0
        tile (th, tw) of every channel c:  += sigma(b, c, tile) * (eta(s0) or its transpose, per (b, tile))
        x_best = x_new = clip(x + D0 / (1e-12 + ||D0||) * eps, lo, hi)                                        nd_square_l2_init
    query i, per ACTIVE row (margin_min > 0), D = x_best - x:                                                 nd_square_l2_propose
        windows w1 = (vh1, vw1), w2 = (vh2, vw2), both of side s = side_l2(i)
        sign sigma_c per channel; transpose bit t
        S_w1  = sum_{w1} D^2
        S_all = sum D^2
        S_mask = sum_{w1 u w2} D^2        # an element in both windows counts once
        S_out = sum_{outside w1 u w2} D^2
        n_w1 = sqrt(S_w1); n_img = sqrt(S_all); n_mask = sqrt(S_mask)
        u = sigma_c * eta_t(s)[i, j] + D[w1] / (1e-12 + n_w1);  S_u = sum u^2;  n_u = sqrt(S_u)
        scale = sqrt(max(eps*eps - n_img*n_img, 0) / Cin + n_mask*n_mask)
        D' = D;  D'[w2] = 0;  D'[w1] = u / (1e-12 + n_u) * scale        # w1 wins where the windows overlap
        S_new = sum_{w1} D'^2;  n' = sqrt(S_out + S_new)
        x_new = clip(x + D' / (1e-12 + n') * eps, lo, hi)
    accept / bookkeeping: exactly nd_square_accept (loss = margin; improved = loss < loss_min; accept = improved or margin <= 0)
    commit: accepted rows: x_best = x_new (whole image); nothing else                                         nd_square_l2_commit

perturb, restarts, generate_attack, check_every, trace, the frozen-row convention and p_selection are those of SquareAttack.
Deviations of the L2 form, documented:
  - autoattack draws one pair of windows, one sign per channel and one eta orientation for the whole batch; here every image draws its
    own from Philox keyed on (seed, the image's global index, query or tile, restart).
  - each sign and each transpose comes from one random bit, where autoattack takes a uniform draw (and, at the start, a random choice).
  - the tile origin: the start tiles nh x nw whole tiles of side s0 centred in the image (margins of (H - nh*s0)//2 rows and
    (W - nw*s0)//2 columns stay 0), where autoattack's h//s loop starts at the corner and assumes a side of 5 * s0; side_l2's last min
    is this project's clamp for images that are not square or smaller than the schedule's window.
  - rejected rows are not restored: x_new keeps the rejected candidate, and the next propose rewrites the whole image from x_best.
  - on a target whose forward is random (an EnsembleTarget without fix_noise()) every query is a fresh draw of the defence: the margin
    a candidate is accepted on is one sample, as it is for autoattack on a randomized model.
Images below 5 x 5 have no start (s0 = 0) and are refused.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, Optional, Tuple

import numpy as np
import torch

from . import ops
from .attack import BOUNDS, _vit


class SquareAttack:
    """autoattack's SquareAttack, Linf and the margin loss, untargeted: perturb(x, y) -> the adversarial batch, and the surface of the
    other attacks here (attack_type, generate_attack) so that attack.apply_attack, Diffusion.test_atk(attack=...) and
    make_attacks.write_attacked_set take it.  `index` (perturb / attack_single_run): the global image index of each row, which keys its
    draws.  check_every: how often the host asks whether any row is still active (0: never)."""

    attack_type = "SQUARE"

    def __init__(self, predict, norm="Linf", n_queries=5000, eps=None, p_init=.8, n_restarts=1, seed=0, verbose=False, targeted=False,
                 loss="margin", resc_schedule=True, device=None, check_every=50):
        if norm != "Linf":
            raise NotImplementedError(f"Square norm '{norm}' is not implemented here (only Linf; the L2 form is square.SquareL2Attack)")
        if loss != "margin":
            raise NotImplementedError(f"Square loss '{loss}' is not implemented (only 'margin')")
        if targeted:
            raise NotImplementedError("targeted Square (targeted=True) is not implemented")
        if eps is None:
            raise ValueError("eps is required")
        if int(n_queries) < 1 or int(check_every) < 0:
            raise ValueError("n_queries must be at least 1 and check_every at least 0")
        model = _vit(predict)
        forward = getattr(model, "forward", model)
        if not callable(forward):
            raise TypeError("predict must be a VisionTransformer, a GuidingConditioner or a callable [B, Cin, H, W] -> [B, C]")
        self.model, self.predict = model, forward
        self.norm, self.n_queries, self.eps, self.p_init, self.n_restarts = norm, int(n_queries), float(eps), float(p_init), int(n_restarts)
        self.epsilon = self.eps                                    # the name the other attacks (and write_attacked_set) use
        self.seed = 0 if seed is None else int(seed)
        self.verbose, self.targeted, self.loss, self.rescale_schedule = verbose, False, loss, bool(resc_schedule)
        self.device = device if device is not None else getattr(model, "device", None)
        self.check_every = int(check_every)

    def p_selection(self, it: int) -> float:
        """The fraction of the image a window covers at query `it` (autoattack's piecewise-constant schedule)."""
        if self.rescale_schedule:
            it = int(it / self.n_queries * 10000)
        for k, (lo, hi) in enumerate(((10, 50), (50, 200), (200, 500), (500, 1000), (1000, 2000), (2000, 4000), (4000, 6000), (6000, 8000),
                                      (8000, math.inf)), start=1):
            if lo < it <= hi:
                return self.p_init / 2 ** k
        return self.p_init

    def side(self, it: int, H: int, W: int) -> int:
        """The window's side at query `it` on H x W images; the min with H and W is this project's clamp for non-square images."""
        return min(max(int(round(math.sqrt(self.p_selection(it) * H * W))), 1), H, W)

    def _scores(self, x: torch.Tensor) -> torch.Tensor:
        scores = self.predict(x)
        if not torch.is_tensor(scores) or scores.dim() != 2 or scores.shape[0] != x.shape[0] or scores.dtype != torch.float32:
            raise ValueError("predict must return a float32 [B, C] tensor")
        return scores

    def attack_single_run(self, x: torch.Tensor, y: torch.Tensor, index: torch.Tensor, restart: int = 0,
                          trace: Optional[Callable] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(n_queries, x_best) of one run from the stripe start.  trace(i, scores, arrays, state), if given, is called after the start
        (i = -1) and after each query's commit; arrays = dict of x_best, x_new and state = the ops.SquareState."""
        eps, seed = self.eps, self.seed
        B, _, H, W = x.shape
        x_best, x_new = ops.square_init(x, index, eps, seed, restart, *BOUNDS)
        st = ops.SquareState(B, x.device)
        scores = self._scores(x_new)
        ops.square_accept(scores, y, st, -1)
        arrays = dict(x_best=x_best, x_new=x_new)
        if trace is not None:
            trace(-1, scores, arrays, st)
        for i in range(self.n_queries):
            if self.check_every and i % self.check_every == 0 and int((st.margin_min > 0).sum()) == 0:
                break                                              # the loop's only read-back: no row is active any more
            s = self.side(i, H, W)
            ops.square_propose(x, x_best, x_new, index, st, s, i, eps, seed, restart, *BOUNDS)
            scores = self._scores(x_new)
            ops.square_accept(scores, y, st, i)
            ops.square_commit(x_best, x_new, st, s)
            if trace is not None:
                trace(i, scores, arrays, st)
        return st.n_queries, x_best

    def perturb(self, x: torch.Tensor, y: torch.Tensor, index: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The adversarial batch: rows the clean model already misclassifies and rows no restart fools come back unchanged."""
        dev = self.device if self.device is not None else x.device
        x = x.to(dev, torch.float32).contiguous()
        y = y.to(dev, torch.int64).contiguous()
        index = (torch.arange(x.shape[0]) if index is None else index).to(dev, torch.int64)
        adv = x.clone()
        if x.shape[0] == 0:
            return adv
        scores = self._scores(x)
        n_cls = scores.shape[1]
        if int(y.min()) < 0 or int(y.max()) >= n_cls:              # once, so that the queries need not read the labels back
            raise ValueError(f"labels must lie in [0, {n_cls})")
        acc = scores.argmax(dim=1) == y
        for r in range(self.n_restarts):
            ind = acc.nonzero().flatten()
            if ind.numel() == 0:
                break
            y_curr = y[ind].contiguous()
            _, adv_curr = self.attack_single_run(x[ind].contiguous(), y_curr, index[ind].contiguous(), restart=r)
            fooled = self._scores(adv_curr).argmax(dim=1) != y_curr
            acc[ind[fooled]] = False
            adv[ind[fooled]] = adv_curr[fooled]
        return adv

    def generate_attack(self, samples: torch.Tensor, labels: torch.Tensor, first_image: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
        """(adversarial images, success), as the other attacks; first_image is the global index of samples[0]."""
        dev = self.device if self.device is not None else samples.device
        labels = labels.to(dev, torch.int64).contiguous()
        index = first_image + torch.arange(samples.shape[0], dtype=torch.int64)
        adv = self.perturb(samples, labels, index=index)
        success = self._scores(adv).argmax(dim=1) != labels if adv.shape[0] else torch.zeros(0, dtype=torch.bool, device=adv.device)
        return adv, success


def eta_rectangles(a: int, b: int) -> np.ndarray:
    """The listing's eta_rectangles in float64: nested centred rectangles weighted 1 / (k + 1)^2, unit L2 norm."""
    d = np.zeros((a, b), dtype=np.float64)
    xc, yc = a // 2 + 1, b // 2 + 1
    c2 = [xc - 1, yc - 1]
    for k in range(max(xc, yc)):
        d[max(c2[0], 0):min(c2[0] + 2 * k + 1, a), max(c2[1], 0):min(c2[1] + 2 * k + 1, b)] += 1.0 / (k + 1) ** 2
        c2[0] -= 1
        c2[1] -= 1
    return d / np.sqrt((d ** 2).sum())


def eta_pattern(s: int) -> np.ndarray:
    """The listing's eta(s): float32 [s, s] of unit L2 norm, computed in float64 and rounded once."""
    d = np.zeros((s, s), dtype=np.float64)
    if s // 2:
        d[:s // 2] = eta_rectangles(s // 2, s)
    d[s // 2:] = -eta_rectangles(s - s // 2, s)
    return (d / np.sqrt((d ** 2).sum())).astype(np.float32)


class SquareL2Attack(SquareAttack):
    """autoattack's SquareAttack with norm='L2' and the margin loss, untargeted, on the nd_square_l2_* kernels: the surface of
    SquareAttack (perturb, attack_single_run, generate_attack, attack_type, epsilon), the same schedule, restarts and frozen-row
    convention.  eta(s) is built on the host once per side and kept on the device."""

    attack_type = "SQUAREL2"
    MIN_DIM = 5

    def __init__(self, predict, n_queries=5000, eps=None, p_init=.8, n_restarts=1, seed=0, verbose=False, resc_schedule=True, device=None,
                 check_every=50):
        # the parent checks and stores everything the two forms share; its norm argument names the Linf form only
        super().__init__(predict, norm="Linf", n_queries=n_queries, eps=eps, p_init=p_init, n_restarts=n_restarts, seed=seed, verbose=verbose,
                         resc_schedule=resc_schedule, device=device, check_every=check_every)
        self.norm = "L2"
        self._eta: Dict[Tuple[int, str], torch.Tensor] = {}

    def side(self, it: int, H: int, W: int) -> int:
        """side_l2 of the listing: odd, at least 3, at most the largest odd number <= min(H, W)."""
        s = max(int(round(math.sqrt(self.p_selection(it) * H * W))), 3)
        s += 1 - s % 2
        m = min(H, W)
        return min(s, m - 1 + m % 2)

    def eta(self, s: int, device=None) -> torch.Tensor:
        """eta(s) as float32 [s, s] on `device` (None: the host), cached per (s, device)."""
        key = (int(s), str(device))
        if key not in self._eta:
            t = torch.from_numpy(eta_pattern(int(s)))
            self._eta[key] = t if device is None else t.to(device)
        return self._eta[key]

    @classmethod
    def check_size(cls, H: int, W: int) -> None:
        if min(H, W) < cls.MIN_DIM:
            raise ValueError(f"SquareL2Attack needs images of at least {cls.MIN_DIM} x {cls.MIN_DIM} (got {H} x {W}): the start tiles "
                             "the image with squares of side min(H, W) // 5")

    def attack_single_run(self, x: torch.Tensor, y: torch.Tensor, index: torch.Tensor, restart: int = 0,
                          trace: Optional[Callable] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(n_queries, x_best) of one run from the tiled start.  trace(i, scores, arrays, state), if given, is called after the start
        (i = -1) and after each query's commit; arrays = dict of x_best, x_new and init_sums (sum D0^2 [B]); state = the
        ops.SquareL2State, whose win and sums are those of the query."""
        eps, seed = self.eps, self.seed
        B, Cin, H, W = x.shape
        self.check_size(H, W)
        x_best, x_new, init_sums = ops.square_l2_init(x, index, self.eta(min(H, W) // 5, x.device), eps, seed, restart, *BOUNDS)
        st = ops.SquareL2State(B, Cin, H, W, x.device)
        scores = self._scores(x_new)
        ops.square_accept(scores, y, st, -1)
        arrays = dict(x_best=x_best, x_new=x_new, init_sums=init_sums)
        if trace is not None:
            trace(-1, scores, arrays, st)
        for i in range(self.n_queries):
            if self.check_every and i % self.check_every == 0 and int((st.margin_min > 0).sum()) == 0:
                break                                              # the loop's only read-back: no row is active any more
            s = self.side(i, H, W)
            ops.square_l2_propose(x, x_best, x_new, index, st, self.eta(s, x.device), s, i, eps, seed, restart, *BOUNDS)
            scores = self._scores(x_new)
            ops.square_accept(scores, y, st, i)
            ops.square_l2_commit(x_best, x_new, st)
            if trace is not None:
                trace(i, scores, arrays, st)
        return st.n_queries, x_best

    def perturb(self, x: torch.Tensor, y: torch.Tensor, index: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The adversarial batch, as SquareAttack.perturb; images below 5 x 5 are refused before the model is called."""
        if x.dim() == 4:
            self.check_size(x.shape[2], x.shape[3])
        return super().perturb(x, y, index=index)
