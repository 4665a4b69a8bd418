"""Host-side pieces of the L2 Square attack (nested_diffusion_amd/square.py SquareL2Attack, csrc/nd_square_l2.hip) and of
autoattack.WorstCase, no GPU needed: eta and the window schedule, the constructor and its refusals, the C ABI declarations and argument
checks, the two float32 restatements of the loop checked against each other, the worst-case runner on fake attacks, and the parser.

ref_l2_init, ref_l2_propose and ref_l2_commit transcribe the listing of include/nested_diffusion.h kernel by kernel in numpy float32, one
operation per rounding, on the Philox words of oracle.ref_cpu.philox4x32_10; tests/test_gpu_square_l2.py imports them as its oracle and
hands them the sums the kernels report (`given=True`).  Without given sums they use sum32: the exact sum of the fp32 terms, rounded once.
HostSquareL2 is written independently, as whole-array masked torch operations in the style of autoattack's square.py (it compacts the
batch to the rows not yet fooled and multiplies by 0/1 masks where the restatement slices), and shares nothing with them but the Philox
words, eta and sum32."""
import argparse
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from oracle import ref_cpu
from test_square_host import ACCEPT, ACTIVE, NO_MODEL, _key, ref_accept, ref_new_state, same, synthetic_scores

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L2_SYMBOLS = ["nd_square_l2_ws_floats", "nd_square_l2_init", "nd_square_l2_propose", "nd_square_l2_commit"]
L2_INIT_TAG, L2_STEP_TAG, L2_SIGN_TAG = 0x53324931, 0x53325331, 0x53324731
S_W1, S_ALL, S_MASK, S_OUT, S_U, S_NEW = range(6)
f32 = np.float32
TINY = f32(1e-12)


# ---- the per-kernel numpy restatement (the GPU tests' oracle) --------------------------------------------------------------------------
def sum32(terms):
    """The exact sum of the fp32 terms, rounded once to fp32."""
    return f32(math.fsum(np.asarray(terms, dtype=np.float64).ravel().tolist()))


def clip32(v, lo, hi):
    return np.fmin(np.fmax(v, f32(lo)), f32(hi))


def ref_l2_new_state(B):
    st = ref_new_state(B)
    st["win"] = np.zeros((B, 4), np.int32)
    st["sums"] = np.zeros((6, B), f32)
    return st


def ref_l2_d0(index, eta0, Cin, H, W, seed, restart):
    """D0 [B, Cin, H, W] of nd_square_l2_init: +-eta(s0), or its transpose, on the centred tiling; 0 on the margins."""
    eta0 = np.asarray(eta0, dtype=f32)
    s0 = min(H, W) // 5
    assert eta0.shape == (s0, s0)
    nh, nw = H // s0, W // s0
    oh, ow = (H - nh * s0) // 2, (W - nw * s0) // 2
    d0 = np.zeros((len(index), Cin, H, W), f32)
    for b, image in enumerate(index):
        ctr = [[int(image) & 0xFFFFFFFF, t, restart, L2_INIT_TAG] for t in range(nh * nw)]
        q = ref_cpu.philox4x32_10(np.asarray(ctr, dtype=np.uint64), *_key(seed))
        for th in range(nh):
            for tw in range(nw):
                q0, q1 = int(q[th * nw + tw][0]), int(q[th * nw + tw][1])
                tile = eta0.T if q1 >> 31 else eta0
                for c in range(Cin):
                    sigma = f32(1.0) if (q0 >> c) & 1 else f32(-1.0)
                    d0[b, c, oh + th * s0:oh + (th + 1) * s0, ow + tw * s0:ow + (tw + 1) * s0] = sigma * tile
    return d0


def ref_l2_init(x0, index, eta0, eps, seed, restart=0, lo=0.0, hi=1.0, sums=None, terms=None):
    """nd_square_l2_init: (x_best, x_new, sums [B]).  sums given: the kernel's, used as they are; terms (a list): receives each row's
    fp32 terms of sum D0^2."""
    x0 = np.asarray(x0, dtype=f32)
    B, Cin, H, W = x0.shape
    d0 = ref_l2_d0(index, eta0, Cin, H, W, seed, restart)
    out = np.zeros(B, f32) if sums is None else np.asarray(sums, dtype=f32)
    v = np.empty_like(x0)
    for b in range(B):
        sq = d0[b] * d0[b]
        if terms is not None:
            terms.append(sq.ravel().copy())
        if sums is None:
            out[b] = sum32(sq)
        den = TINY + np.sqrt(out[b])
        v[b] = clip32(x0[b] + (d0[b] / den) * f32(eps), lo, hi)
    return v.copy(), v.copy(), out


def ref_l2_draw(image, it, seed, restart, H, W, s):
    """(vh1, vw1, vh2, vw2, sign word, transpose) of one row's query."""
    p = ref_cpu.philox4x32_10([[int(image) & 0xFFFFFFFF, it, restart, L2_STEP_TAG]], *_key(seed))[0]
    q = ref_cpu.philox4x32_10([[int(image) & 0xFFFFFFFF, it, restart, L2_SIGN_TAG]], *_key(seed))[0]
    v = [(int(p[0]) * (H - s + 1)) >> 32, (int(p[1]) * (W - s + 1)) >> 32, (int(p[2]) * (H - s + 1)) >> 32, (int(p[3]) * (W - s + 1)) >> 32]
    return (*v, int(q[0]), bool(int(q[1]) >> 31))


def ref_l2_propose(x0, x_best, x_new, index, margin_min, eta, win, sums, s, it, eps, seed, restart=0, lo=0.0, hi=1.0, given=False,
                   terms=None, draw=None):
    """nd_square_l2_propose, in place on x_new, win and (unless given) sums [6, B].  given: sums holds the kernel's six sums, used as
    they are.  terms (a dict): terms[b] = the fp32 terms of each of the six sums of row b.  draw(b) overrides a row's Philox draw."""
    B, Cin, H, W = x0.shape
    eta = np.asarray(eta, dtype=f32)
    assert eta.shape == (s, s)
    e = f32(eps)
    for b in range(B):
        if not margin_min[b] > 0:
            continue
        vh1, vw1, vh2, vw2, bits, transpose = draw(b) if draw is not None else ref_l2_draw(index[b], it, seed, restart, H, W, s)
        win[b] = (vh1, vw1, vh2, vw2)
        w1 = (slice(None), slice(vh1, vh1 + s), slice(vw1, vw1 + s))
        w2 = (slice(None), slice(vh2, vh2 + s), slice(vw2, vw2 + s))
        D = x_best[b] - x0[b]
        sq = D * D
        mask = np.zeros((H, W), bool)
        mask[w1[1:]] = True
        mask[w2[1:]] = True
        S = sums[:, b]
        t = {S_W1: sq[w1], S_ALL: sq, S_MASK: sq[:, mask], S_OUT: sq[:, ~mask]}
        if not given:
            for k in (S_W1, S_ALL, S_MASK, S_OUT):
                S[k] = sum32(t[k])
        den_w1 = TINY + np.sqrt(S[S_W1])
        sigma = np.array([1.0 if (bits >> c) & 1 else -1.0 for c in range(Cin)], f32).reshape(Cin, 1, 1)
        u = sigma * (eta.T if transpose else eta)[None] + D[w1] / den_w1
        t[S_U] = u * u
        if not given:
            S[S_U] = sum32(t[S_U])
        den_u = TINY + np.sqrt(S[S_U])
        n_img, n_mask = np.sqrt(S[S_ALL]), np.sqrt(S[S_MASK])
        scale = np.sqrt(np.fmax(e * e - n_img * n_img, f32(0.0)) / f32(Cin) + n_mask * n_mask)
        Dn = D.copy()
        Dn[w2] = f32(0.0)
        Dn[w1] = (u / den_u) * scale                               # w1 wins where the windows overlap
        t[S_NEW] = Dn[w1] * Dn[w1]
        if not given:
            S[S_NEW] = sum32(t[S_NEW])
        den = TINY + np.sqrt(S[S_OUT] + S[S_NEW])
        x_new[b] = clip32(x0[b] + (Dn / den) * e, lo, hi)
        if terms is not None:
            terms[b] = {k: np.asarray(v, dtype=f32).ravel().copy() for k, v in t.items()}


def ref_l2_commit(x_best, x_new, flags):
    """nd_square_l2_commit, in place on x_best."""
    for b in range(x_best.shape[0]):
        if int(flags[b]) & (ACTIVE | ACCEPT) == (ACTIVE | ACCEPT):
            x_best[b] = x_new[b]


# ---- the independent whole-array restatement -------------------------------------------------------------------------------------------
class HostSquareL2:
    """attack_single_run with norm='L2' as whole-array torch float32 operations in autoattack's style, fed the scores of each query."""

    def __init__(self, x, y, index, eps, seed, restart, eta_of):
        self.x, self.y, self.index = x.float().clone(), y.long().clone(), [int(i) for i in index]
        self.eps, self.seed, self.restart, self.eta_of = torch.tensor(eps, dtype=torch.float32), seed, restart, eta_of

    def _words(self, counter):
        w = ref_cpu.philox4x32_10(np.asarray([counter], dtype=np.uint64), self.seed % 2 ** 32, (self.seed // 2 ** 32) % 2 ** 32)
        return w[0].astype(np.int64).tolist()

    @staticmethod
    def lp_sq(t):
        """per image: the sum of squares over everything but the batch axis (sum32 of the fp32 squares), as a [n, 1, 1, 1] tensor"""
        sq = (t * t).reshape(t.shape[0], -1)
        return torch.tensor([float(sum32(row.numpy())) for row in sq], dtype=torch.float32).view(-1, 1, 1, 1)

    @staticmethod
    def root(t):
        """The correctly rounded fp32 square root (numpy's; torch's CPU sqrt is a 0.5001-ulp approximation and misses near-ties)."""
        return torch.from_numpy(np.sqrt(t.numpy()))

    @staticmethod
    def margin_and_loss(scores, y):
        u = torch.arange(scores.shape[0])
        logits = scores.clone()
        y_corr = logits[u, y].clone()
        logits[u, y] = -float("inf")
        margin = y_corr - logits.max(dim=-1)[0]
        return margin, margin.clone()

    def init(self, scores):
        B, C, H, W = self.x.shape
        s0 = min(H, W) // 5
        eta0 = self.eta_of(s0)
        nh, nw = H // s0, W // s0
        oh, ow = (H - nh * s0) // 2, (W - nw * s0) // 2
        delta = torch.zeros_like(self.x)
        for b, image in enumerate(self.index):
            for t in range(nh * nw):
                q = self._words([image % 2 ** 32, t, self.restart, L2_INIT_TAG])
                signs = torch.tensor([2.0 * ((q[0] // 2 ** c) % 2) - 1.0 for c in range(C)]).view(C, 1, 1)
                pattern = eta0.t() if q[1] // 2 ** 31 else eta0
                h0, w0 = oh + (t // nw) * s0, ow + (t % nw) * s0
                delta[b, :, h0:h0 + s0, w0:w0 + s0] += pattern.view(1, s0, s0) * signs
        self.init_sq = self.lp_sq(delta)
        self.x_best = torch.clamp(self.x + delta / (1e-12 + self.root(self.init_sq)) * self.eps, 0.0, 1.0)
        self.margin_min, self.loss_min = self.margin_and_loss(scores, self.y)
        self.n_queries = torch.ones(B, dtype=torch.int32)

    def query(self, i, s, scores):
        """One query; returns the rows it ran on, their candidates, their corners and whether each was accepted."""
        B, C, H, W = self.x.shape
        idx = (self.margin_min > 0.0).nonzero().flatten()
        x_curr, x_best_curr, y_curr = self.x[idx], self.x_best[idx], self.y[idx]
        n = idx.numel()
        delta_curr = x_best_curr - x_curr
        mask_1, mask_2 = torch.zeros(n, 1, H, W), torch.zeros(n, 1, H, W)
        pattern, corners = torch.zeros(n, C, H, W), []
        eta = self.eta_of(s)
        for r, b in enumerate(idx.tolist()):
            p = self._words([self.index[b] % 2 ** 32, i, self.restart, L2_STEP_TAG])
            q = self._words([self.index[b] % 2 ** 32, i, self.restart, L2_SIGN_TAG])
            vh1, vw1, vh2, vw2 = (p[0] * (H - s + 1) // 2 ** 32, p[1] * (W - s + 1) // 2 ** 32, p[2] * (H - s + 1) // 2 ** 32,
                                  p[3] * (W - s + 1) // 2 ** 32)
            mask_1[r, :, vh1:vh1 + s, vw1:vw1 + s] = 1.0
            mask_2[r, :, vh2:vh2 + s, vw2:vw2 + s] = 1.0
            signs = torch.tensor([2.0 * ((q[0] // 2 ** c) % 2) - 1.0 for c in range(C)]).view(C, 1, 1)
            pattern[r, :, vh1:vh1 + s, vw1:vw1 + s] = (eta.t() if q[1] // 2 ** 31 else eta).view(1, s, s) * signs
            corners.append((vh1, vw1, vh2, vw2))
        mask_image = torch.max(mask_1, mask_2)
        sq_window_1 = self.lp_sq(delta_curr * mask_1)
        sq_image = self.lp_sq(delta_curr)
        sq_windows = self.lp_sq(delta_curr * mask_image)
        sq_outside = self.lp_sq(delta_curr * (1.0 - mask_image))
        new_deltas = (pattern + delta_curr / (1e-12 + self.root(sq_window_1))) * mask_1
        sq_u = self.lp_sq(new_deltas)
        n_img, n_mask = self.root(sq_image), self.root(sq_windows)
        channels = torch.full_like(n_img, float(C))                # a full tensor: a true division per row, not a multiply by 1 / C
        scale = self.root(torch.clamp(self.eps * self.eps - n_img * n_img, min=0.0) / channels + n_mask * n_mask)
        new_deltas = new_deltas / (1e-12 + self.root(sq_u)) * scale
        delta_new = delta_curr * (1.0 - mask_image) + new_deltas * mask_1
        sq_new = self.lp_sq(delta_new * mask_1)
        x_new = torch.clamp(x_curr + delta_new / (1e-12 + self.root(sq_outside + sq_new)) * self.eps, 0.0, 1.0)
        margin, loss = self.margin_and_loss(scores[idx], y_curr)
        loss_min_curr = self.loss_min[idx]
        idx_improved = loss < loss_min_curr
        self.loss_min[idx] = torch.where(idx_improved, loss, loss_min_curr)
        idx_improved = idx_improved | (margin <= 0.0)
        self.margin_min[idx] = torch.where(idx_improved, margin, self.margin_min[idx])
        self.x_best[idx] = torch.where(idx_improved.view(-1, 1, 1, 1), x_new, x_best_curr)
        self.n_queries[idx] += 1
        sums = torch.cat([t.view(1, -1) for t in (sq_window_1, sq_image, sq_windows, sq_outside, sq_u, sq_new)])
        return idx, x_new, corners, idx_improved, sums


# ---- eta and the sides -----------------------------------------------------------------------------------------------------------------
def make(**kw):
    from nested_diffusion_amd.square import SquareL2Attack
    kw.setdefault("eps", 0.5)
    return SquareL2Attack(NO_MODEL, **kw)


def test_eta_values_and_norm():
    a = make()
    want3 = np.array([[.13608276, .68041382, .13608276], [-.12909944, -.12909944, -.12909944], [-.12909944, -.64549722, -.12909944]])
    assert a.eta(3).dtype == torch.float32 and tuple(a.eta(3).shape) == (3, 3)
    # the listing's values carry 8 decimals (+-5e-9); eta is rounded once to fp32 (half an ulp below 1: 2^-25)
    assert np.abs(a.eta(3).numpy().astype(np.float64) - want3).max() <= 5e-9 + 2.0 ** -25
    same("eta(1)", a.eta(1), np.array([[-1.0]], f32))
    for s in (1, 3, 5, 9, 44, 201):
        e = a.eta(s).numpy().astype(np.float64)
        assert e.shape == (s, s) and abs(math.sqrt((e ** 2).sum()) - 1.0) < s * 2.0 ** -24, s     # every entry rounded once: <= 2^-25 relative
        assert (e[:s // 2] > 0).all() and (e[s // 2:] < 0).all()
    assert a.eta(9) is a.eta(9)                                                                    # cached


def test_side_l2():
    a = make(n_queries=5000)
    its = [0, 11, 51, 201, 501, 1001, 2001, 4001, 6001, 8001]
    assert [a.side(i, 224, 224) for i in its] == [201, 143, 101, 71, 35, 25, 19, 9, 9, 9]
    assert [a.side(i, 8, 8) for i in its] == [7, 5, 5, 3, 3, 3, 3, 3, 3, 3]
    assert [a.side(i, 5, 5) for i in its] == [5] + [3] * 9
    for H, W in ((32, 48), (48, 32)):
        sides = {a.side(i, H, W) for i in range(10000)}
        assert all(s % 2 == 1 and 3 <= s <= 31 for s in sides) and 31 in sides and 3 in sides, sides


# ---- constructor and surface -----------------------------------------------------------------------------------------------------------
def test_constructor_surface_and_refusals():
    import inspect
    from nested_diffusion_amd.square import SquareAttack, SquareL2Attack
    sig = inspect.signature(SquareL2Attack.__init__)
    names = list(sig.parameters)[1:]
    assert names == ["predict", "n_queries", "eps", "p_init", "n_restarts", "seed", "verbose", "resc_schedule", "device", "check_every"]
    assert [sig.parameters[n].default for n in names[1:]] == [5000, None, .8, 1, 0, False, True, None, 50]
    a = make(eps=0.5)
    assert (a.norm, a.attack_type, SquareL2Attack.attack_type, a.eps, a.epsilon, a.n_queries, a.p_init, a.n_restarts, a.seed, a.check_every) == \
        ("L2", "SQUAREL2", "SQUAREL2", 0.5, 0.5, 5000, .8, 1, 0, 50)
    for method in ("side", "eta", "attack_single_run", "perturb", "generate_attack", "p_selection"):
        assert callable(getattr(a, method)), method
    assert "trace" in inspect.signature(a.attack_single_run).parameters and "index" in inspect.signature(a.perturb).parameters
    assert "first_image" in inspect.signature(a.generate_attack).parameters
    vit = types.SimpleNamespace(device="cpu", forward=lambda x: x)
    assert SquareL2Attack(vit, eps=0.1).predict is vit.forward and SquareL2Attack(types.SimpleNamespace(vit=vit), eps=0.1).model is vit
    with pytest.raises(ValueError, match="eps"):
        SquareL2Attack(NO_MODEL)
    with pytest.raises(TypeError, match="callable"):
        SquareL2Attack(types.SimpleNamespace(device="cpu"), eps=0.1)
    with pytest.raises(ValueError, match="n_queries"):
        SquareL2Attack(NO_MODEL, eps=0.1, n_queries=0)
    # images below 5 x 5 are refused by name, before the model is called
    for shape in ((2, 3, 4, 8), (2, 3, 8, 4)):
        with pytest.raises(ValueError, match=r"SquareL2Attack needs images of at least 5 x 5"):
            a.perturb(torch.zeros(shape), torch.zeros(2, dtype=torch.int64))
    # the Linf class still refuses the L2 norm, and now says where it lives
    with pytest.raises(NotImplementedError, match=r"L2.*square\.SquareL2Attack"):
        SquareAttack(NO_MODEL, eps=0.1, norm="L2")
    assert SquareAttack(NO_MODEL, eps=0.1).attack_type == "SQUARE"


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
def test_header_signatures_and_tags():
    from nested_diffusion_amd import _lib, build, ops
    with open(os.path.join(ROOT, "include", "nested_diffusion.h")) as f:
        hdr = f.read()
    for s in L2_SYMBOLS:
        assert re.search(rf"\b(int|size_t) {s}\(", hdr), s
        assert s in _lib.SIGNATURES, s
    for name in ("square_l2_init", "square_l2_propose", "square_l2_commit", "SquareL2State", "square_accept"):
        assert hasattr(ops, name), name
    tags = {n: int(v, 16) for n, v in re.findall(r"#define (ND_\w+_TAG) (0x[0-9A-Fa-f]+)u", hdr)}
    assert (tags["ND_SQUARE_L2_INIT_TAG"], tags["ND_SQUARE_L2_STEP_TAG"], tags["ND_SQUARE_L2_SIGN_TAG"]) == (L2_INIT_TAG, L2_STEP_TAG, L2_SIGN_TAG)
    assert len(tags) >= 8 and len(set(tags.values())) == len(tags), tags                          # every draw has a tag of its own
    assert f"#define ND_SQUARE_L2_SUMS {ops.SQUARE_L2_SUMS}\n" in hdr
    for k, name in enumerate(("W1", "ALL", "MASK", "OUT", "U", "NEW")):
        assert f"#define ND_SQUARE_L2_S_{name} {k}\n" in hdr
    assert "nd_square_l2.hip" in build.SOURCES
    build.build()
    lib = _lib.load()
    for s in L2_SYMBOLS:
        assert hasattr(lib, s), s
    assert lib.nd_square_l2_ws_floats(3, 224, 224) == lib.nd_square_l2_ws_floats(1, 5, 5) == 6 * 256
    assert lib.nd_square_l2_ws_floats(3, 4, 8) == lib.nd_square_l2_ws_floats(33, 8, 8) == lib.nd_square_l2_ws_floats(3, 8, 4097) == 0
    assert issubclass(ops.SquareL2State, ops.SquareState)


def test_kernels_refuse_bad_arguments_before_any_launch():
    from nested_diffusion_amd import _lib, build
    build.build()
    lib = _lib.load()
    P = 4096                                                       # dummy non-NULL addresses, never dereferenced
    Q, R = 8192, 12288

    def init(x0=P, eta0=P, sums=P, B=2, Cin=3, H=8, W=12, s0=1):
        return lib.nd_square_l2_init(x0, P, eta0, Q, R, sums, P, B, Cin, H, W, s0, 1, 0, 0.5, 0.0, 1.0, None)

    def prop(x0=P, xb=Q, xn=R, eta=P, win=P, sums=P, ws=P, B=2, Cin=3, H=8, W=12, s=5, it=0):
        return lib.nd_square_l2_propose(x0, xb, xn, P, P, eta, win, sums, ws, B, Cin, H, W, s, it, 1, 0, 0.5, 0.0, 1.0, None)

    def com(xb=P, xn=Q, fl=P, B=2, per=192):
        return lib.nd_square_l2_commit(xb, xn, fl, B, per, None)

    cases = [
        (lambda: init(x0=None), rb"NULL tensor"), (lambda: init(eta0=None), rb"NULL tensor"), (lambda: init(sums=None), rb"NULL tensor"),
        (lambda: init(B=0), rb"square L2 init needs 1 <= B <= 65535 \(B=0\)"), (lambda: init(B=65536), rb"1 <= B <= 65535 \(B=65536\)"),
        (lambda: init(Cin=0), rb"1 <= Cin <= 32 \(Cin=0\)"), (lambda: init(Cin=33), rb"1 <= Cin <= 32 \(Cin=33\)"),
        (lambda: init(H=4), rb"5 <= H, W <= 4096 \(H=4, W=12\)"), (lambda: init(W=4097, s0=1), rb"5 <= H, W <= 4096"),
        (lambda: init(s0=2), rb"s0 = min\(H, W\) / 5 \(s0=2, H=8, W=12\)"), (lambda: init(H=10, W=10, s0=1), rb"s0 = min\(H, W\) / 5"),
        (lambda: prop(x0=None), rb"NULL tensor"), (lambda: prop(eta=None), rb"NULL tensor"), (lambda: prop(win=None), rb"NULL tensor"),
        (lambda: prop(sums=None), rb"NULL tensor"), (lambda: prop(ws=None), rb"NULL tensor"),
        (lambda: prop(B=0), rb"square L2 propose needs 1 <= B <= 65535"), (lambda: prop(Cin=33), rb"1 <= Cin <= 32 \(Cin=33\)"),
        (lambda: prop(H=4), rb"5 <= H, W <= 4096 \(H=4, W=12\)"),
        (lambda: prop(s=4), rb"an odd s, 3 <= s <= min\(H, W\) \(s=4, H=8, W=12\)"), (lambda: prop(s=1), rb"an odd s, 3 <= s"),
        (lambda: prop(s=9), rb"3 <= s <= min\(H, W\) \(s=9, H=8, W=12\)"), (lambda: prop(H=12, W=8, s=9), rb"3 <= s <= min\(H, W\)"),
        (lambda: prop(it=-1), rb"square L2 propose needs iter >= 0 \(iter=-1\)"),
        (lambda: prop(xn=P), rb"three arrays"), (lambda: prop(xn=Q), rb"three arrays"),
        (lambda: com(xb=None), rb"NULL tensor"), (lambda: com(fl=None), rb"NULL tensor"), (lambda: com(B=0), rb"square L2 commit needs 1 <= B <= 65535"),
        (lambda: com(per=24), rb"25 <= per_image"), (lambda: com(xn=P), rb"two arrays"),
    ]
    for n, (call, msg) in enumerate(cases):
        assert call() == -1, (n, msg)                              # ND_ERR_ARG
        assert re.search(msg, lib.nd_last_error()), (n, msg, lib.nd_last_error())


# ---- the two restatements agree ----------------------------------------------------------------------------------------------------------
def test_l2_restatements_agree_bit_for_bit_on_a_synthetic_run():
    """ref_l2_init / ref_l2_propose / ref_accept / ref_l2_commit against HostSquareL2 over 120 queries of B = 24 images of 3 x 12 x 20
    with 3 classes, sides 11, 7, 5 and 3 (the production schedule): every array, every sum and every state vector after every query."""
    B, Cin, H, W, C, n_queries, eps, seed, restart = 24, 3, 12, 20, 3, 120, 0.75, (7 << 32) | 11, 2
    atk = make(eps=eps, n_queries=n_queries)
    sides = [atk.side(i, H, W) for i in range(n_queries)]
    assert sides[0] == 11 and sides[-1] == 3 and sorted(set(sides), reverse=True) == [11, 7, 5, 3]
    eta_np = lambda s: atk.eta(s).numpy()                          # noqa: E731
    rng = np.random.default_rng(2025)
    x = rng.random((B, Cin, H, W), dtype=f32)
    x[rng.random(x.shape) < 0.1] = 0.0
    x[rng.random(x.shape) < 0.1] = 1.0
    y = rng.integers(0, C, B)
    index = (np.arange(B, dtype=np.int64) * 3 + 1000)
    index[3] = (1 << 31) + 17                                      # above 2^31
    index[4] = (5 << 32) + 9                                       # only the low word keys the draw
    level = np.full(B, 1.5, f32)

    sc = synthetic_scores(rng, B, C, y, level, first=True)
    host = HostSquareL2(torch.from_numpy(x), torch.from_numpy(y), index, eps, seed, restart, atk.eta)
    host.init(torch.from_numpy(sc))
    x_best, x_new, init_sums = ref_l2_init(x, index, eta_np(min(H, W) // 5), eps, seed, restart)
    same("init sums", host.init_sq.flatten(), init_sums)
    # 6 x 10 tiles of side 2 cover the image: every element carries +-eta(2), so sum D0^2 = 60 * Cin * ||eta(2)||^2
    assert np.abs(init_sums - 60 * Cin).max() < 1e-3 and not np.array_equal(x_best, x)
    st = ref_l2_new_state(B)
    ref_accept(sc, y, st, -1)

    def compare(where):
        same("x_best", host.x_best, x_best, where)
        for n in ("margin_min", "loss_min", "n_queries"):
            same(n, getattr(host, n), st[n], where)

    compare("after the start")
    d64 = (x_best.astype(np.float64) - x).reshape(B, -1)
    assert (np.sqrt((d64 ** 2).sum(1)) <= eps * (1 + 1e-5)).all()
    frozen_at_start = ~(st["margin_min"] > 0)
    assert frozen_at_start[5] and frozen_at_start[6] and frozen_at_start[7]
    start_best = x_best.copy()
    seen, overlaps, active_queries = set(), set(), np.zeros(B, np.int64)
    for i in range(n_queries):
        s = sides[i]
        active = st["margin_min"] > 0
        active_queries += active
        sc = synthetic_scores(rng, B, C, y, level, first=False)
        win_before, sums_before, new_before = st["win"].copy(), st["sums"].copy(), x_new.copy()
        ref_l2_propose(x, x_best, x_new, index, st["margin_min"], eta_np(s), st["win"], st["sums"], s, i, eps, seed, restart)
        idx, cand, corners, accepted, sums = host.query(i, s, torch.from_numpy(sc))
        where = f"query {i}"
        assert idx.tolist() == np.flatnonzero(active).tolist()
        same("candidate", cand, x_new[active], where)
        same("win", torch.tensor(corners, dtype=torch.int32).reshape(-1, 4), st["win"][active], where)
        same("sums", sums, st["sums"][:, active], where)
        same("win of the frozen rows", st["win"][~active], win_before[~active], where)
        same("sums of the frozen rows", st["sums"][:, ~active], sums_before[:, ~active], where)
        same("x_new of the frozen rows", x_new[~active], new_before[~active], where)
        for vh1, vw1, vh2, vw2 in corners:
            dh, dw = abs(vh1 - vh2), abs(vw1 - vw2)
            overlaps.add("same" if (dh, dw) == (0, 0) else "partial" if dh < s and dw < s else "disjoint")
        # the candidate lies on or inside the eps-sphere (clipping to [0, 1] only shrinks it)
        d64 = (x_new[active].astype(np.float64) - x[active]).reshape(int(active.sum()), -1)
        assert (np.sqrt((d64 ** 2).sum(1)) <= eps * (1 + 1e-5)).all(), where
        ref_accept(sc, y, st, i)
        want_flags = np.zeros(B, np.int32)
        want_flags[active] = ACTIVE | (accepted.numpy().astype(np.int32) * ACCEPT)
        same("flags", st["flags"], want_flags, where)
        ref_l2_commit(x_best, x_new, st["flags"])
        compare(f"after query {i}")
        seen |= set(int(v) for v in st["flags"])
    assert seen == {0, ACTIVE, ACTIVE | ACCEPT}
    assert {"partial", "disjoint"} <= overlaps
    frozen = ~(st["margin_min"] > 0)
    assert (frozen & ~frozen_at_start).sum() >= B // 4 and (~frozen).sum() >= B // 4
    same("n_queries", st["n_queries"], (1 + active_queries).astype(np.int32))
    same("x_best of the rows frozen at the start", x_best[frozen_at_start], start_best[frozen_at_start])
    assert x_best.min() >= 0.0 and x_best.max() <= 1.0


def test_restatement_edge_cases_stay_finite():
    """w1 = w2, D = 0 on w1, x_best = x0 everywhere and ||x_best - x0|| > eps (the max(., 0) branch): no zero denominator, and the
    candidate stays inside the ball."""
    atk = make(eps=0.5)
    rng = np.random.default_rng(5)
    B, Cin, H, W, s = 4, 3, 8, 8, 3
    x = (0.25 + 0.5 * rng.random((B, Cin, H, W), dtype=f32)).astype(f32)
    x_best = x.copy()                                              # row 0: x_best = x0 everywhere
    x_best[1] = x[1] + f32(0.01)
    x_best[1, :, 2:5, 1:4] = x[1, :, 2:5, 1:4]                     # row 1: D = 0 on w1
    x_best[2] = x[2] + f32(0.2)                                    # row 2: ||D|| = 0.2 * sqrt(192) > eps
    x_best[3] = x[3] + (rng.random((Cin, H, W), dtype=f32) - f32(0.5)) * f32(0.05)
    draws = {0: (2, 1, 2, 1, 0b101, False), 1: (2, 1, 5, 5, 0b010, True), 2: (5, 5, 4, 4, 0b111, False), 3: (0, 0, 5, 5, 0, True)}
    x_new, win, sums = np.zeros_like(x), np.zeros((B, 4), np.int32), np.zeros((6, B), f32)
    ref_l2_propose(x, x_best, x_new, np.arange(B), np.ones(B, f32), atk.eta(s).numpy(), win, sums, s, 0, 0.5, 1, draw=lambda b: draws[b])
    assert np.isfinite(x_new).all() and np.isfinite(sums).all()
    assert sums[S_W1, 0] == 0 and sums[S_ALL, 0] == 0 and sums[S_W1, 1] == 0 and sums[S_ALL, 1] > 0
    assert float(np.sqrt(sums[S_ALL, 2])) > 0.5
    same("S_mask = S_w1 where the windows coincide", sums[S_MASK, 0:1], sums[S_W1, 0:1])
    d = (x_new.astype(np.float64) - x).reshape(B, -1)
    norms = np.sqrt((d ** 2).sum(1))
    assert (norms <= 0.5 * (1 + 1e-5)).all() and (norms > 0.49).all(), norms          # on the sphere: nothing here is clipped by [0, 1]
    assert win.tolist() == [list(draws[b][:4]) for b in range(B)]


# ---- the worst-case runner ---------------------------------------------------------------------------------------------------------------
class FakeAttack:
    """Fools the rows whose global index is in `fools` by painting them black (class 1 for the model below); records its calls."""

    def __init__(self, name, fools, norm="L2", eps=0.5):
        self.attack_type, self.fools, self.norm, self.eps, self.calls = name, set(fools), norm, eps, []

    def perturb(self, x, y, index=None):
        self.calls.append((x.clone(), y.clone(), index.clone()))
        out = x.clone()
        for r, i in enumerate(index.tolist()):
            out[r] = 0.0 if i in self.fools else x[r] * 0.999
        return out


def mean_model(x):
    """class 0 iff the image's mean exceeds 0.5"""
    m = x.flatten(1).mean(1)
    return torch.stack([m, 0.5 + 0 * m], dim=1)


def test_worst_case_order_indices_and_first_adversarial():
    from nested_diffusion_amd import attack
    from nested_diffusion_amd.autoattack import WorstCase
    x = torch.full((8, 3, 6, 6), 0.75)
    x[2] = 0.25                                                    # the clean model gets row 2 wrong
    y = torch.zeros(8, dtype=torch.int64)
    a1, a2, a3 = FakeAttack("A1", {101, 104}), FakeAttack("A2", {101, 105, 107}), FakeAttack("A3", {100})
    wc = WorstCase(mean_model, [a1, a2, a3])
    assert (wc.attack_type, WorstCase.attack_type, wc.norm, wc.eps, wc.epsilon, wc.model) == ("WORSTCASE", "WORSTCASE", "L2", 0.5, 0.5, mean_model)
    x_in = x.clone()
    adv = wc.perturb(x, y, index=100 + torch.arange(8))
    assert torch.equal(x, x_in)
    # each attack saw only the rows still robust, with their global indices, in order
    assert [c[2].tolist() for c in a1.calls] == [[100, 101, 103, 104, 105, 106, 107]]
    assert [c[2].tolist() for c in a2.calls] == [[100, 103, 105, 106, 107]]
    assert [c[2].tolist() for c in a3.calls] == [[100, 103, 106]]
    assert a2.calls[0][2].dtype == torch.int64 and torch.equal(a2.calls[0][0], x[[0, 3, 5, 6, 7]]) and a2.calls[0][1].tolist() == [0] * 5
    assert wc.robust_after == [("clean", 7), ("A1", 5), ("A2", 3), ("A3", 2)]
    fooled = [0, 1, 4, 5, 7]
    assert float(adv[fooled].abs().max()) == 0.0
    for r in (2, 3, 6):                                            # wrong when clean, and never fooled: unchanged (not the 0.999 x a member returned)
        assert torch.equal(adv[r], x[r])
    # the first adversarial found is kept: A2 would also fool 101, but never sees it
    assert 101 not in a2.calls[0][2].tolist()
    # generate_attack / apply_attack
    adv2, success = wc.generate_attack(x, y, first_image=100)
    assert torch.equal(adv2, adv) and success.tolist() == [True, True, True, False, True, True, False, True]
    assert torch.equal(attack.apply_attack(wc, x, y, wc.attack_type, first_image=100), adv)
    # all rows fooled by the first attack: the later ones are not called
    b1, b2 = FakeAttack("B1", set(range(8))), FakeAttack("B2", set())
    wc2 = WorstCase(mean_model, [b1, b2])
    wc2.perturb(x, y)
    assert b1.calls[0][2].tolist() == [0, 1, 3, 4, 5, 6, 7] and b2.calls == [] and wc2.robust_after == [("clean", 7), ("B1", 0)]


def test_worst_case_refusals():
    from nested_diffusion_amd.autoattack import AutoAttack, WorstCase
    with pytest.raises(ValueError, match=r"A1 has norm='L2', eps=0.5 and A2 has norm='Linf', eps=0.5"):
        WorstCase(mean_model, [FakeAttack("A1", ()), FakeAttack("A2", (), norm="Linf")])
    with pytest.raises(ValueError, match=r"A1 has norm='L2', eps=0.5 and A2 has norm='L2', eps=0.25"):
        WorstCase(mean_model, [FakeAttack("A1", ()), FakeAttack("A2", (), eps=0.25)])
    with pytest.raises(ValueError, match="at least one"):
        WorstCase(mean_model, [])
    with pytest.raises(TypeError, match="perturb"):
        WorstCase(mean_model, [types.SimpleNamespace(norm="L2", eps=0.5)])
    # the L2 evaluation is built from the two real classes; AutoAttack still refuses norm='L2' by name
    from nested_diffusion_amd.autoattack import APGDAttack
    from nested_diffusion_amd.square import SquareL2Attack
    vit = types.SimpleNamespace(device="cpu", forward=mean_model)
    wc = WorstCase(vit, [APGDAttack(vit, norm="L2", eps=0.5), SquareL2Attack(vit, eps=0.5)])
    assert (wc.norm, wc.eps, [a.attack_type for a in wc.attacks]) == ("L2", 0.5, ["APGD", "SQUAREL2"]) and wc.model is vit
    with pytest.raises(NotImplementedError, match="L2"):
        AutoAttack(vit, norm="L2", eps=0.5, version="custom", attacks_to_run=["apgd-ce"])


# ---- the parser --------------------------------------------------------------------------------------------------------------------------
def test_parser_namespace_unchanged_and_n_queries_refusal(tmp_path):
    from nested_diffusion_amd import make_attacks
    base = ["--config", "c.yml", "--eps", "0.5", "--out", "o"]
    a = make_attacks.build_parser().parse_args(base + ["--attack_name", "APGDL2"])
    assert vars(a) == dict(config="c.yml", attack_name="APGDL2", eps=0.5, out="o", preprocess="grayscaled", seed=0, batch_size=32, dataroot=None,
                           device=0, target="vit", members=None)
    for name in ("SQUARE", "SQUAREL2"):
        b = make_attacks.build_parser().parse_args(base + ["--attack_name", name])
        assert b.attack_name == name and not hasattr(b, "n_queries")
        c = make_attacks.build_parser().parse_args(base + ["--attack_name", name, "--n_queries", "300"])
        assert c.n_queries == 300
        make_attacks.check_n_queries(c)
        atk = make_attacks.make_named_attack(c, NO_MODEL)
        assert (atk.attack_type, atk.n_queries, atk.eps, atk.norm) == (name, 300, 0.5, "L2" if name == "SQUAREL2" else "Linf")
        assert make_attacks.make_named_attack(b, NO_MODEL).n_queries == 5000
    # refused by name before the config is opened: the config path does not exist
    missing = str(tmp_path / "missing.yml")
    for name in ("PGD", "APGDL2", "AUTOPGD"):
        with pytest.raises(SystemExit, match="--n_queries"):
            make_attacks.main(["--config", missing, "--eps", "0.5", "--out", "o", "--attack_name", name, "--n_queries", "10"])
    with pytest.raises(SystemExit, match=r"--n_queries must be at least 1"):
        make_attacks.main(["--config", missing, "--eps", "0.5", "--out", "o", "--attack_name", "SQUAREL2", "--n_queries", "0"])
    assert isinstance(make_attacks.build_parser(), argparse.ArgumentParser)
