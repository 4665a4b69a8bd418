"""Host-side pieces of the Square attack (nested_diffusion_amd/square.py, csrc/nd_square.hip), no GPU needed: the window schedule, the
constructor and its refusals, the surface attack.apply_attack drives, the C ABI declarations and argument checks of the four kernels, and
the two float32 restatements of the loop checked against each other.

ref_init, ref_propose, ref_accept and ref_commit transcribe the listing of include/nested_diffusion.h kernel by kernel in numpy float32,
one operation per rounding, on the Philox words of oracle.ref_cpu.philox4x32_10; tests/test_gpu_square.py imports them as its oracle.
HostSquare is written independently, as whole-array torch operations in the style of autoattack's square.py (it compacts the batch to the
rows not yet fooled, clones x_best per query and clamps the whole array), and shares nothing with them but the Philox words."""
import math
import os
import re

import numpy as np
import pytest
import torch

from oracle import ref_cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SQUARE_SYMBOLS = ["nd_square_init", "nd_square_propose", "nd_square_accept", "nd_square_commit"]
INIT_TAG, STEP_TAG = 0x53514931, 0x53515331
ACTIVE, ACCEPT = 1, 2
f32 = np.float32
NO_MODEL = lambda x: None                                          # noqa: E731  (a predict that is never called)


# ---- the per-kernel numpy restatement (the GPU tests' oracle) --------------------------------------------------------------------------
def _key(seed):
    return seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF


def ref_new_state(B):
    """Poisoned, as the tests poison the device state before the initialising call."""
    return dict(margin_min=np.full(B, np.nan, f32), loss_min=np.full(B, np.nan, f32), n_queries=np.full(B, 0x7FFFFFFF, np.int32),
                flags=np.full(B, 0x7FFFFFFF, np.int32), win=np.zeros((B, 2), np.int32))


def ref_sigma(index, Cin, W, seed, restart):
    """[B, Cin, 1, W] of +-1: the top bit of word j % 4 of philox(index[b], j / 4, restart, INIT_TAG), j = c * W + w."""
    index = np.asarray(index, dtype=np.int64)
    B, n = index.shape[0], Cin * W
    j = np.arange(n)
    b, jj = np.meshgrid(index & 0xFFFFFFFF, j, indexing="ij")
    ctr = np.stack([b, jj // 4, np.full_like(jj, restart), np.full_like(jj, INIT_TAG)], axis=-1).reshape(-1, 4)
    words = ref_cpu.philox4x32_10(ctr, *_key(seed)).reshape(B, n, 4)
    word = words[np.arange(B)[:, None], j[None, :], (j % 4)[None, :]]
    return np.where((word >> np.uint32(31)) != 0, f32(1.0), f32(-1.0)).astype(f32).reshape(B, Cin, 1, W)


def ref_init(x0, index, eps, seed, restart=0, lo=0.0, hi=1.0):
    """nd_square_init: (x_best, x_new)."""
    x0 = np.asarray(x0, dtype=f32)
    _, Cin, _, W = x0.shape
    d = f32(eps) * ref_sigma(index, Cin, W, seed, restart)
    v = np.minimum(np.maximum(x0 + d, f32(lo)), f32(hi))
    return v.copy(), v.copy()


def ref_draw(image, it, seed, restart, H, W, s):
    """(vh, vw, sign word) of one row's query."""
    p = ref_cpu.philox4x32_10([[int(image) & 0xFFFFFFFF, it, restart, STEP_TAG]], *_key(seed))[0]
    vh = (int(p[0]) * (H - s + 1)) >> 32
    vw = (int(p[1]) * (W - s + 1)) >> 32
    return vh, vw, int(p[2])


def ref_propose(x0, x_best, x_new, index, margin_min, win, s, it, eps, seed, restart=0, lo=0.0, hi=1.0):
    """nd_square_propose, in place on x_new and win."""
    B, Cin, H, W = x0.shape
    e = f32(eps)
    two = e + e
    for b in range(B):
        if not margin_min[b] > 0:
            continue
        vh, vw, bits = ref_draw(index[b], it, seed, restart, H, W, s)
        for c in range(Cin):
            d = two if (bits >> c) & 1 else -two
            sl = (b, c, slice(vh, vh + s), slice(vw, vw + s))
            x = x0[sl]
            x_new[sl] = np.minimum(np.maximum(np.minimum(np.maximum(x_best[sl] + d, x - e), x + e), f32(lo)), f32(hi))
        win[b] = (vh, vw)


def ref_margin(row, y):
    row = np.asarray(row, dtype=f32)
    if np.isnan(row).any() or not 0 <= y < row.shape[0]:
        return f32(np.nan)
    with np.errstate(invalid="ignore"):
        return f32(row[y] - np.delete(row, y).max())


def ref_accept(scores, labels, st, it):
    """nd_square_accept on the state dict st, in place."""
    scores = np.asarray(scores, dtype=f32)
    for b in range(scores.shape[0]):
        if it >= 0 and not st["margin_min"][b] > 0:
            st["flags"][b] = 0
            continue
        margin = ref_margin(scores[b], int(labels[b]))
        loss = margin
        if it < 0:
            st["margin_min"][b], st["loss_min"][b], st["n_queries"][b], st["flags"][b] = margin, loss, 1, 0
            continue
        improved = bool(loss < st["loss_min"][b])
        if improved:
            st["loss_min"][b] = loss
        accept = improved or bool(margin <= 0)
        if accept:
            st["margin_min"][b] = margin
        st["n_queries"][b] += 1
        st["flags"][b] = ACTIVE | (ACCEPT if accept else 0)


def ref_commit(x_best, x_new, win, flags, s):
    """nd_square_commit, in place on x_best and x_new."""
    for b in range(x_best.shape[0]):
        f = int(flags[b])
        if not f & ACTIVE:
            continue
        vh, vw = int(win[b, 0]), int(win[b, 1])
        if vh < 0 or vw < 0 or vh > x_best.shape[2] - s or vw > x_best.shape[3] - s:
            continue                                               # a corner that does not keep the window inside the image is ignored
        sl = (b, slice(None), slice(vh, vh + s), slice(vw, vw + s))
        if f & ACCEPT:
            x_best[sl] = x_new[sl]
        else:
            x_new[sl] = x_best[sl]


# ---- helpers ---------------------------------------------------------------------------------------------------------------------------
def bits(t):
    t = t.detach().cpu() if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t))
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(name, got, want, where=""):
    """bit for bit (the int32 view of floats: NaN payloads and signed zeros count); names the first element that differs."""
    g, w = bits(got), bits(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (name, where, g.shape, w.shape, g.dtype, w.dtype)
    if not torch.equal(g, w):
        bad = (g != w).nonzero()
        at = tuple(bad[0].tolist())
        gv = got.detach().cpu()[at] if torch.is_tensor(got) else got[at]
        wv = want.detach().cpu()[at] if torch.is_tensor(want) else want[at]
        raise AssertionError(f"{name} {where}: {bad.shape[0]} of {g.numel()} elements differ, the first at {at}: got {gv!r}, want {wv!r}")


# ---- the independent whole-array restatement -------------------------------------------------------------------------------------------
class HostSquare:
    """attack_single_run as whole-array torch float32 operations in autoattack's style, fed the scores of each query."""

    def __init__(self, x, y, index, eps, seed, restart=0):
        self.x, self.y, self.index = x.float().clone(), y.long().clone(), [int(i) for i in index]
        self.eps, self.seed, self.restart = torch.tensor(eps, dtype=torch.float32), seed, restart

    def _words(self, counters):
        w = ref_cpu.philox4x32_10(np.asarray(counters, dtype=np.uint64), self.seed % 2 ** 32, (self.seed // 2 ** 32) % 2 ** 32)
        return torch.from_numpy(w.astype(np.int64))

    @staticmethod
    def margin_and_loss(scores, y):
        u = torch.arange(scores.shape[0])
        logits = scores.clone()
        y_corr = logits[u, y].clone()
        logits[u, y] = -float("inf")
        y_others = logits.max(dim=-1)[0]                           # torch.max propagates a NaN among the others
        margin = y_corr - y_others
        return margin, margin.clone()

    def init(self, scores):
        B, C, H, W = self.x.shape
        stripes = torch.empty(B, C, 1, W)
        for b, image in enumerate(self.index):
            quads = self._words([[image % 2 ** 32, q, self.restart, INIT_TAG] for q in range((C * W + 3) // 4)])
            top = (quads.flatten()[:C * W] // 2 ** 31) % 2          # the top bit of the j-th word of the row's stream of quads
            stripes[b] = (2.0 * top.float() - 1.0).view(C, 1, W)
        self.x_best = torch.clamp(self.x + self.eps * stripes, 0.0, 1.0)
        self.margin_min, self.loss_min = self.margin_and_loss(scores, self.y)
        self.n_queries = torch.ones(B, dtype=torch.int32)

    def query(self, i, s, scores):
        """One query; returns what the per-kernel restatement exposes for comparison: the rows it ran on, their candidate images,
        their window corners and whether each was accepted."""
        B, C, H, W = self.x.shape
        idx = (self.margin_min > 0.0).nonzero().flatten()
        x_curr, x_best_curr, y_curr = self.x[idx], self.x_best[idx], self.y[idx]
        x_new = x_best_curr.clone()
        corners = []
        for r, b in enumerate(idx.tolist()):
            w = self._words([[self.index[b] % 2 ** 32, i, self.restart, STEP_TAG]])[0].tolist()
            vh, vw = w[0] * (H - s + 1) // 2 ** 32, w[1] * (W - s + 1) // 2 ** 32
            signs = torch.tensor([2.0 * ((w[2] // 2 ** c) % 2) - 1.0 for c in range(C)]).view(C, 1, 1)
            x_new[r, :, vh:vh + s, vw:vw + s] = x_best_curr[r, :, vh:vh + s, vw:vw + s] + (2.0 * self.eps) * signs
            corners.append((vh, vw))
        x_new = torch.min(torch.max(x_new, x_curr - self.eps), x_curr + self.eps)
        x_new = torch.clamp(x_new, 0.0, 1.0)
        margin, loss = self.margin_and_loss(scores[idx], y_curr)
        loss_min_curr = self.loss_min[idx]
        idx_improved = loss < loss_min_curr
        self.loss_min[idx] = torch.where(idx_improved, loss, loss_min_curr)
        idx_miscl = margin <= 0.0
        idx_improved = idx_improved | idx_miscl
        self.margin_min[idx] = torch.where(idx_improved, margin, self.margin_min[idx])
        self.x_best[idx] = torch.where(idx_improved.view(-1, 1, 1, 1), x_new, x_best_curr)
        self.n_queries[idx] += 1
        return idx, x_new, corners, idx_improved


# ---- schedule and sides ----------------------------------------------------------------------------------------------------------------
ITS = [0, 10, 11, 50, 51, 200, 201, 500, 1000, 2000, 4000, 6000, 8000, 8001, 9999]
# the exponent k of p = p_init / 2^k at those (rescaled) iterations: the boundaries belong to the interval below them
KS = [0, 0, 1, 1, 2, 2, 3, 3, 4, 5, 6, 7, 8, 9, 9]
EDGES = [10, 50, 200, 500, 1000, 2000, 4000, 6000, 8000]


@pytest.mark.parametrize("n_queries", [5000, 1000])
def test_p_selection(n_queries):
    from nested_diffusion_amd.square import SquareAttack
    raw = SquareAttack(NO_MODEL, eps=0.1, n_queries=n_queries, resc_schedule=False, p_init=0.8)
    assert [raw.p_selection(it) for it in ITS] == [0.8 / 2 ** k for k in KS]
    resc = SquareAttack(NO_MODEL, eps=0.1, n_queries=n_queries, p_init=0.8)
    for it in ITS:                                                 # rescaled first: it -> int(it / n_queries * 10000), then the same table
        v = int(it / n_queries * 10000)
        assert resc.p_selection(it) == 0.8 / 2 ** sum(v > edge for edge in EDGES), (it, v)
    # spot values: with 5000 queries iteration 5 is rescaled to 10 (p_init), 6 to 12 (half), 4001 to 8002 (1 / 512)
    a = SquareAttack(NO_MODEL, eps=0.1, n_queries=5000, p_init=0.8)
    assert (a.p_selection(5), a.p_selection(6), a.p_selection(25), a.p_selection(26), a.p_selection(4001)) == \
        (0.8, 0.4, 0.4, 0.2, 0.8 / 512)
    b = SquareAttack(NO_MODEL, eps=0.1, n_queries=1000, p_init=0.8)
    assert (b.p_selection(1), b.p_selection(2), b.p_selection(5), b.p_selection(6), b.p_selection(999)) == (0.8, 0.4, 0.4, 0.2, 0.8 / 512)


def test_side():
    from nested_diffusion_amd.square import SquareAttack
    a = SquareAttack(NO_MODEL, eps=0.1, n_queries=5000, p_init=0.8, resc_schedule=False)
    assert a.side(0, 224, 224) == 200 and a.side(10, 224, 224) == 200
    assert a.side(11, 224, 224) == 142                             # the side after it = 10: p = 0.4
    assert a.side(0, 32, 48) == 32                                 # sqrt(0.8 * 32 * 48) = 35: clamped to the shorter edge
    assert a.side(0, 48, 32) == 32
    tiny = SquareAttack(NO_MODEL, eps=0.1, p_init=1e-6, resc_schedule=False)
    assert tiny.side(0, 224, 224) == 1 and tiny.side(9999, 8, 8) == 1
    assert a.side(9999, 224, 224) == int(round(math.sqrt(0.8 / 512 * 224 * 224))) == 9
    # Python's round: halves go to the even neighbour (sqrt(0.25 * 25) = 2.5 -> 2)
    assert SquareAttack(NO_MODEL, eps=0.1, p_init=0.25, resc_schedule=False).side(0, 5, 5) == 2


# ---- constructor and surface -----------------------------------------------------------------------------------------------------------
def test_constructor_defaults_and_refusals():
    import inspect
    import types
    from nested_diffusion_amd.square import SquareAttack
    sig = inspect.signature(SquareAttack.__init__)
    names = list(sig.parameters)[1:]
    assert names[:12] == ["predict", "norm", "n_queries", "eps", "p_init", "n_restarts", "seed", "verbose", "targeted", "loss",
                          "resc_schedule", "device"]
    d = {n: sig.parameters[n].default for n in names[1:]}
    assert (d["norm"], d["n_queries"], d["eps"], d["p_init"], d["n_restarts"], d["seed"], d["verbose"], d["targeted"], d["loss"],
            d["resc_schedule"], d["device"], d["check_every"]) == ("Linf", 5000, None, .8, 1, 0, False, False, "margin", True, None, 50)
    a = SquareAttack(NO_MODEL, eps=8 / 255)
    assert a.attack_type == "SQUARE" and SquareAttack.attack_type == "SQUARE"
    assert (a.norm, a.n_queries, a.eps, a.epsilon, a.p_init, a.n_restarts, a.seed, a.loss, a.rescale_schedule, a.check_every) == \
        ("Linf", 5000, 8 / 255, 8 / 255, .8, 1, 0, "margin", True, 50)
    assert a.model is NO_MODEL and a.predict is NO_MODEL
    assert SquareAttack(NO_MODEL, eps=0.1, seed=None).seed == 0
    # a VisionTransformer is called through forward; a GuidingConditioner is accepted for its ViT
    vit = types.SimpleNamespace(device="cpu", forward=lambda x: x)
    assert SquareAttack(vit, eps=0.1).predict is vit.forward and SquareAttack(vit, eps=0.1).device == "cpu"
    assert SquareAttack(types.SimpleNamespace(vit=vit), eps=0.1).model is vit
    for kwargs, match in ((dict(norm="L2"), "L2"), (dict(norm="L1"), "L1"), (dict(loss="ce"), "'ce'"), (dict(targeted=True), "targeted")):
        with pytest.raises(NotImplementedError, match=match):
            SquareAttack(NO_MODEL, eps=0.1, **kwargs)
    with pytest.raises(ValueError, match="eps"):
        SquareAttack(NO_MODEL)
    with pytest.raises(TypeError, match="callable"):
        SquareAttack(types.SimpleNamespace(device="cpu"), eps=0.1)


def test_autoattack_still_refuses_square_and_names_the_class():
    import types
    from nested_diffusion_amd.autoattack import AutoAttack
    fake = types.SimpleNamespace(device="cpu")
    with pytest.raises(NotImplementedError, match=r"'square'.*square\.SquareAttack"):
        AutoAttack(fake, eps=0.1, version="custom", attacks_to_run=["square"])
    with pytest.raises(NotImplementedError, match="standard"):
        AutoAttack(fake, eps=0.1, version="standard")


def test_apply_attack_drives_generate_attack():
    from nested_diffusion_amd import attack
    from nested_diffusion_amd.square import SquareAttack
    calls = []
    scores = lambda x: torch.stack([x.flatten(1).mean(1), 0.5 + 0 * x.flatten(1).mean(1)], dim=1)   # noqa: E731  class 0 iff the mean > 0.5

    class Fake(SquareAttack):
        def perturb(self, x, y, index=None):
            calls.append((x, y, index))
            out = x.clone()
            out[::2] = 0.0                                         # the even rows become all black: class 1
            return out

    x = torch.full((5, 3, 4, 4), 0.75)
    y = torch.zeros(5, dtype=torch.int64)
    atk = Fake(scores, eps=0.1, n_queries=3)
    x_in = x.clone()
    out = attack.apply_attack(atk, x, y, atk.attack_type, first_image=40)
    (cx, cy, index), = calls
    assert torch.equal(cx, x_in) and cx is not x and torch.equal(x, x_in)                       # the inputs are not modified
    assert torch.equal(cy, y) and index.dtype == torch.int64 and index.tolist() == [40, 41, 42, 43, 44]
    assert torch.equal(out[1::2], x[1::2]) and float(out[::2].abs().max()) == 0.0
    adv, success = atk.generate_attack(x, y, first_image=0)
    assert success.tolist() == [True, False, True, False, True] and torch.equal(adv, out)
    # the labels are range-checked once, on the host, before any kernel runs
    with pytest.raises(ValueError, match=r"labels must lie in \[0, 2\)"):
        SquareAttack(scores, eps=0.1, n_queries=3).generate_attack(x, torch.tensor([0, 1, 2, 0, 0]))
    # nothing to attack: every row is misclassified already, so no kernel is needed and the batch comes back unchanged
    adv, success = SquareAttack(scores, eps=0.1, n_queries=3).generate_attack(x, torch.ones(5, dtype=torch.int64))
    assert torch.equal(adv, x) and success.all()


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
def test_header_and_signatures_carry_the_square_entry_points():
    from nested_diffusion_amd import _lib, build, ops
    with open(os.path.join(ROOT, "include", "nested_diffusion.h")) as f:
        hdr = f.read()
    for s in SQUARE_SYMBOLS:
        assert re.search(rf"\bint {s}\(", hdr), s
        assert s in _lib.SIGNATURES, s
        assert hasattr(ops, s[3:]), s
    assert f"ND_SQUARE_INIT_TAG 0x{INIT_TAG:08X}u" in hdr and f"ND_SQUARE_STEP_TAG 0x{STEP_TAG:08X}u" in hdr
    tags = re.findall(r"#define (ND_\w+_TAG) (0x[0-9A-Fa-f]+)u", hdr)
    assert len(tags) >= 5 and len({int(v, 16) for _, v in tags}) == len(tags), tags             # every draw has a tag of its own
    for name, v in (("ACTIVE", ACTIVE), ("ACCEPT", ACCEPT)):
        assert f"ND_SQUARE_{name} {v}" in hdr and getattr(ops, f"SQUARE_{name}") == v
    assert "nd_square.hip" in build.SOURCES
    build.build()
    lib = _lib.load()
    for s in SQUARE_SYMBOLS:
        assert hasattr(lib, s), s


def test_square_kernels_refuse_bad_arguments_before_any_launch():
    from nested_diffusion_amd import _lib, build
    build.build()
    lib = _lib.load()
    P = 4096                                                       # a dummy non-NULL address, never dereferenced
    init = lambda x0=P, idx=P, xb=P, xn=P, B=2, Cin=3, H=8, W=8: lib.nd_square_init(x0, idx, xb, xn, B, Cin, H, W, 1, 0, 0.1, 0.0, 1.0, None)   # noqa: E731
    prop = lambda x0=P, win=P, B=2, Cin=3, H=8, W=12, s=4, it=0: lib.nd_square_propose(x0, P, P, P, P, win, B, Cin, H, W, s, it, 1, 0, 0.1, 0.0, 1.0, None)   # noqa: E731
    acc = lambda sc=P, fl=P, B=2, C=3, it=0: lib.nd_square_accept(sc, P, P, P, P, fl, B, C, it, None)   # noqa: E731
    com = lambda xb=P, fl=P, B=2, Cin=3, H=8, W=12, s=4: lib.nd_square_commit(xb, P, P, fl, B, Cin, H, W, s, None)   # noqa: E731
    cases = [
        (lambda: init(x0=None), rb"NULL tensor"), (lambda: init(idx=None), rb"NULL tensor"), (lambda: init(xn=None), rb"NULL tensor"),
        (lambda: init(B=0), rb"square init needs 1 <= B <= 65535 \(B=0\)"), (lambda: init(B=65536), rb"1 <= B <= 65535 \(B=65536\)"),
        (lambda: init(Cin=0), rb"1 <= Cin <= 32 \(Cin=0\)"), (lambda: init(Cin=33), rb"1 <= Cin <= 32 \(Cin=33\)"),
        (lambda: init(H=0), rb"1 <= H, W"), (lambda: init(W=0), rb"1 <= H, W"),
        (lambda: prop(x0=None), rb"NULL tensor"), (lambda: prop(win=None), rb"NULL tensor"),
        (lambda: prop(B=0), rb"square propose needs 1 <= B <= 65535"), (lambda: prop(Cin=33), rb"1 <= Cin <= 32"),
        (lambda: prop(s=0), rb"1 <= s <= min\(H, W\) \(s=0"), (lambda: prop(s=9), rb"1 <= s <= min\(H, W\) \(s=9, H=8, W=12\)"),
        (lambda: prop(H=12, W=8, s=9), rb"1 <= s <= min\(H, W\)"), (lambda: prop(it=-1), rb"square propose needs iter >= 0 \(iter=-1\)"),
        (lambda: acc(sc=None), rb"NULL tensor"), (lambda: acc(fl=None), rb"NULL tensor"),
        (lambda: acc(B=0), rb"square accept needs 1 <= B <= 65535"), (lambda: acc(B=65536), rb"1 <= B <= 65535"),
        (lambda: acc(C=1), rb"2 <= C <= 1024 \(C=1\)"), (lambda: acc(C=1025), rb"2 <= C <= 1024 \(C=1025\)"),
        (lambda: acc(it=-2), rb"iter >= -1 \(iter=-2\)"),
        (lambda: com(xb=None), rb"NULL tensor"), (lambda: com(fl=None), rb"NULL tensor"),
        (lambda: com(B=0), rb"square commit needs 1 <= B <= 65535"), (lambda: com(Cin=0), rb"1 <= Cin <= 32"),
        (lambda: com(s=0), rb"1 <= s <= min\(H, W\)"), (lambda: com(s=9), rb"1 <= s <= min\(H, W\) \(s=9, H=8, W=12\)"),
    ]
    for n, (call, msg) in enumerate(cases):
        assert call() == -1, (n, msg)                              # ND_ERR_ARG
        assert re.search(msg, lib.nd_last_error()), (n, msg, lib.nd_last_error())


# ---- the two restatements agree ----------------------------------------------------------------------------------------------------------
def synthetic_scores(rng, B, C, y, level, first):
    """One query's scores, in quarters (so that ties are common and every margin is exact): the label's score is the runner-up's plus
    the row's level, so the margin is the level.  The levels walk: the lower half of the batch drifts down through zero (those rows
    become fooled at different queries, some exactly at margin 0), the upper half stays at or above a quarter.  NaN entries, +inf at the
    label, and in the lower half -inf at the label and +inf at both the label and the runner-up (a NaN margin) are sprinkled in."""
    half = B // 2
    if not first:
        u = rng.random(B)
        level += np.where(u < 0.55, f32(-0.25), np.where(u < 0.9, f32(0.25), f32(0.0)))
        level[half:] = np.maximum(level[half:], f32(0.25))
    sc = (np.round(rng.standard_normal((B, C)) * 4) / 4).astype(f32)
    rows = np.arange(B)
    sc[rows, y] = -np.inf
    other = sc.max(axis=1)
    sc[rows, y] = other + level
    lower = rows < half
    sc[rows[rng.random(B) < 0.01], rng.integers(0, C)] = np.nan
    hit = rng.random(B) < 0.01
    sc[rows[hit], y[hit]] = np.inf
    hit = (rng.random(B) < 0.004) & lower
    sc[rows[hit], y[hit]] = -np.inf
    hit = (rng.random(B) < 0.004) & lower
    sc[rows[hit]] = np.inf
    if first:
        sc[5, 0] = np.nan                                          # a NaN margin at the start: frozen for the whole run
        sc[6, y[6]] = other[6] - f32(0.5)                          # misclassified at the start
        sc[7] = 0.0
        sc[7, y[7]] = -0.0                                         # margin -0.0 - 0.0 = -0.0 at the start: frozen
    return sc


def test_square_restatements_agree_bit_for_bit_on_a_synthetic_run():
    """ref_init / ref_propose / ref_accept / ref_commit against HostSquare over 200 queries of B = 64 images of 3 x 12 x 20 with
    3 classes, sides from 12 down to 1 (the production schedule): every array and every state vector after every query."""
    from nested_diffusion_amd.square import SquareAttack
    B, Cin, H, W, C, n_queries, eps, seed, restart = 64, 3, 12, 20, 3, 200, 0.05, (7 << 32) | 11, 2
    sched = SquareAttack(NO_MODEL, eps=eps, n_queries=n_queries, p_init=0.8)
    sides = [sched.side(i, H, W) for i in range(n_queries)]
    assert sides[0] == 12 and sides[-1] == 1 and sorted(set(sides), reverse=True) == [12, 10, 7, 5, 3, 2, 1]
    rng = np.random.default_rng(2024)
    x = rng.random((B, Cin, H, W), dtype=f32)
    x[rng.random(x.shape) < 0.1] = 0.0
    x[rng.random(x.shape) < 0.1] = 1.0
    y = rng.integers(0, C, B)
    index = (np.arange(B, dtype=np.int64) * 3 + 1000)
    index[3] = (1 << 31) + 17                                      # above 2^31
    index[4] = (5 << 32) + 9                                       # only the low word keys the draw
    level = np.full(B, 1.5, f32)

    sc = synthetic_scores(rng, B, C, y, level, first=True)
    host = HostSquare(torch.from_numpy(x), torch.from_numpy(y), index, eps, seed, restart)
    host.init(torch.from_numpy(sc))
    x_best, x_new = ref_init(x, index, eps, seed, restart)
    st = ref_new_state(B)
    ref_accept(sc, y, st, -1)

    def compare(where):
        same("x_best", host.x_best, x_best, where)
        same("x_new", x_new, x_best, where)                        # the invariant of the two-array layout
        for n in ("margin_min", "loss_min", "n_queries"):
            same(n, getattr(host, n), st[n], where)

    compare("after the start")
    assert np.isnan(st["margin_min"][5]) and st["margin_min"][6] < 0 and np.signbit(st["margin_min"][7]) and st["margin_min"][7] == 0
    frozen_at_start = ~(st["margin_min"] > 0)
    start_best = x_best.copy()
    seen, active_queries = set(), np.zeros(B, np.int64)
    for i in range(n_queries):
        s = sides[i]
        active = st["margin_min"] > 0
        active_queries += active
        sc = synthetic_scores(rng, B, C, y, level, first=False)
        win_before = st["win"].copy()
        ref_propose(x, x_best, x_new, index, st["margin_min"], st["win"], s, i, eps, seed, restart)
        idx, cand, corners, accepted = host.query(i, s, torch.from_numpy(sc))
        assert idx.tolist() == np.flatnonzero(active).tolist()
        same("candidate", cand, x_new[active], f"query {i}")
        same("win", torch.tensor(corners, dtype=torch.int32).reshape(-1, 2), st["win"][active], f"query {i}")
        same("win of the frozen rows", st["win"][~active], win_before[~active], f"query {i}")
        same("x_new of the frozen rows", x_new[~active], x_best[~active], f"query {i}")
        ref_accept(sc, y, st, i)
        want_flags = np.zeros(B, np.int32)
        want_flags[active] = ACTIVE | (accepted.numpy().astype(np.int32) * ACCEPT)
        same("flags", st["flags"], want_flags, f"query {i}")
        ref_commit(x_best, x_new, st["win"], st["flags"], s)
        compare(f"after query {i}")
        seen |= set(int(v) for v in st["flags"])
    assert seen == {0, ACTIVE, ACTIVE | ACCEPT}                    # the run passed every flag value from accept to commit
    frozen = ~(st["margin_min"] > 0)
    assert frozen.sum() >= B // 4 and (~frozen).sum() >= B // 4, (frozen.sum(), (~frozen).sum())
    assert (frozen & ~frozen_at_start).sum() >= B // 4             # rows that became frozen during the run, at different queries
    assert len(set(active_queries[frozen & ~frozen_at_start].tolist())) >= 4
    same("n_queries", st["n_queries"], (1 + active_queries).astype(np.int32))
    same("x_best of the rows frozen at the start", x_best[frozen_at_start], start_best[frozen_at_start])
    assert np.isnan(st["margin_min"][5]) and (st["margin_min"][frozen & ~np.isnan(st["margin_min"])] <= 0).all()
    assert x_best.min() >= 0.0 and x_best.max() <= 1.0
    e = f32(eps)
    assert (x_best >= np.maximum(x - e, 0)).all() and (x_best <= np.minimum(x + e, 1)).all()
