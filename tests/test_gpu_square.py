"""The Square attack on the GPU (nd_square_* in csrc/nd_square.hip, nested_diffusion_amd/square.py): each kernel alone and the whole loop,
bit for bit (the int32 view of the floats) against the per-kernel numpy restatement of tests/test_square_host.py, which that file checks
against an independently written whole-array version on the CPU.  Every image array and state vector a kernel writes lies inside a larger
buffer with sentinels in front of and behind it, at an address that is not 16-byte aligned; the sentinels are checked after every call."""
import os

import numpy as np
import pytest
import torch

from oracle import ref_cpu
from test_square_host import ACCEPT, ACTIVE, ref_accept, ref_commit, ref_draw, ref_init, ref_new_state, ref_propose, same

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32
EPS = 0.1
SEED = (9 << 32) | 1234
# one image of one channel, a non-square image, rows that are not 16-byte aligned (W = 30), more images than one accept workgroup holds
SHAPES = [(1, 1, 8, 8), (3, 3, 32, 48), (5, 3, 30, 30), (70, 3, 32, 32)]
FRONT, BACK = 255, 257                   # sentinel elements around every guarded array: the live part starts 4 bytes off a 16-byte boundary
F_SENT, I_SENT = 3.0e38, -12345
# margin_min of the rows of a batch, cycled: active rows and every kind of frozen row (<= 0, -0.0, NaN)
MARGINS = [1.0, 0.5, -1.0, -0.0, float("nan"), 2.0, 0.0, 1e-30]


# ---- helpers --------------------------------------------------------------------------------------------------------------------------
class Guarded:
    """A device copy of a numpy array inside a larger buffer of sentinels."""

    def __init__(self, a):
        a = np.ascontiguousarray(a)
        sent = F_SENT if a.dtype == np.float32 else I_SENT
        self.sent, self.n = sent, a.size
        self.buf = torch.full((FRONT + a.size + BACK,), sent, dtype=torch.from_numpy(a).dtype, device=DEV)
        self.t = self.buf[FRONT:FRONT + a.size].view(a.shape)
        self.t.copy_(torch.from_numpy(a))
        assert self.t.is_contiguous() and self.t.data_ptr() % 16 != 0

    def check(self, what):
        assert bool((self.buf[:FRONT] == self.sent).all()) and bool((self.buf[FRONT + self.n:] == self.sent).all()), f"{what}: wrote out of bounds"


def guarded_state(st_np):
    """An ops.SquareState whose arrays are Guarded copies of the dict st_np; returns (state, guards)."""
    from nested_diffusion_amd import ops
    B = st_np["flags"].shape[0]
    st = ops.SquareState(B, DEV)
    guards = {n: Guarded(st_np[n]) for n in ("margin_min", "loss_min", "n_queries", "flags", "win")}
    for n, g in guards.items():
        setattr(st, n, g.t)
    return st, guards


def check_all(guards, what):
    for n, g in guards.items():
        g.check(f"{what}: {n}")


def make_images(B, Cin, H, W, seed=0):
    rng = np.random.default_rng(100 + seed)
    x = rng.random((B, Cin, H, W), dtype=f32)
    x[rng.random(x.shape) < 0.1] = 0.0                              # exact 0.0 and 1.0: the clip to the bounds is active
    x[rng.random(x.shape) < 0.1] = 1.0
    x.flat[0], x.flat[-1] = 0.0, 1.0
    index = np.arange(B, dtype=np.int64) * 7 + 3
    index[0] = (1 << 31) + 5                                       # above 2^31
    if B > 1:
        index[1] = (3 << 32) + 2                                   # only the low word keys the draw
    return x, index


def margins(B):
    return np.array([MARGINS[b % len(MARGINS)] for b in range(B)], dtype=f32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- nd_square_init ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("restart", [0, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_init_matches_the_restatement(shape, restart):
    from nested_diffusion_amd import _lib, ops
    x, index = make_images(*shape)
    want_best, want_new = ref_init(x, index, EPS, SEED, restart)
    x_best, x_new = ops.square_init(dev(x), dev(index), EPS, SEED, restart)
    same("x_best", x_best, want_best)
    same("x_new", x_new, want_new)
    assert torch.equal(x_best, x_new)
    assert float(x_best.min()) >= 0.0 and float(x_best.max()) <= 1.0
    d = want_best - x
    assert (d > 0).any() and (d < 0).any()                         # both signs occur
    # written through guarded, misaligned outputs: nothing outside the arrays is touched
    B, Cin, H, W = shape
    gb, gn, d_x, d_index = Guarded(np.zeros_like(x)), Guarded(np.zeros_like(x)), dev(x), dev(index)
    _lib.check(_lib.load().nd_square_init(d_x.data_ptr(), d_index.data_ptr(), gb.t.data_ptr(), gn.t.data_ptr(), B, Cin, H, W, SEED, restart,
                                          EPS, 0.0, 1.0, torch.cuda.current_stream().cuda_stream), "nd_square_init")
    torch.cuda.synchronize()
    same("x_best (guarded)", gb.t, want_best)
    same("x_new (guarded)", gn.t, want_new)
    gb.check("init x_best")
    gn.check("init x_new")
    if restart:
        assert not np.array_equal(want_best, ref_init(x, index, EPS, SEED, 0)[0])       # a restart draws other stripes


# ---- nd_square_propose and nd_square_commit ---------------------------------------------------------------------------------------------------
def sides_of(shape):
    return sorted({1, 5, 7, min(shape[2], shape[3])})


@pytest.mark.parametrize("restart", [0, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_propose_and_commit_match_the_restatement(shape, restart):
    """Three queries per side on one pair of arrays (windows of consecutive queries overlap), accepts and rejects mixed in the batch,
    frozen rows of every kind among them: after every launch every array against the restatement, the frozen rows against their bits
    before the launch, and after every commit x_new == x_best over the whole arrays."""
    from nested_diffusion_amd import ops
    B, Cin, H, W = shape
    x, index = make_images(*shape)
    x_best, x_new = ref_init(x, index, EPS, SEED, restart)
    st_np = ref_new_state(B)
    st_np["margin_min"] = margins(B)
    st_np["win"][:] = -77                                          # a frozen row's corner is never written
    active = st_np["margin_min"] > 0
    st, guards = guarded_state(st_np)
    gx0, gbest, gnew = Guarded(x), Guarded(x_best), Guarded(x_new)
    guards.update(x0=gx0, x_best=gbest, x_new=gnew)
    d_index = dev(index)
    it = 0
    for s in sides_of(shape):
        for _ in range(3):
            before_best, before_new = x_best.copy(), x_new.copy()
            ops.square_propose(gx0.t, gbest.t, gnew.t, d_index, st, s, it, EPS, SEED, restart)
            ref_propose(x, x_best, x_new, index, st_np["margin_min"], st_np["win"], s, it, EPS, SEED, restart)
            where = f"propose s={s} it={it}"
            same("x_new", gnew.t, x_new, where)
            same("x_best", gbest.t, before_best, where)
            same("win", st.win, st_np["win"], where)
            same("x0", gx0.t, x, where)
            same("x_new of the frozen rows", gnew.t[dev(~active)], before_new[~active], where)
            assert (st_np["win"][~active] == -77).all()
            if s == min(H, W):                                     # the window is the whole image the short way: that corner is 0
                corner = st_np["win"][active]
                assert (corner[:, 0 if H <= W else 1] == 0).all()
            check_all(guards, where)
            flags = np.where(active, ACTIVE | np.where((np.arange(B) + it) % 2 == 0, ACCEPT, 0), 0).astype(np.int32)
            st_np["flags"][:] = flags
            st.flags.copy_(dev(flags))
            before_best, before_new = x_best.copy(), x_new.copy()
            ops.square_commit(gbest.t, gnew.t, st, s)
            ref_commit(x_best, x_new, st_np["win"], st_np["flags"], s)
            where = f"commit s={s} it={it}"
            same("x_best", gbest.t, x_best, where)
            same("x_new", gnew.t, x_new, where)
            assert torch.equal(gnew.t, gbest.t), where             # the invariant, accept and reject rows mixed
            same("x_best of the frozen rows", gbest.t[dev(~active)], before_best[~active], where)
            same("win", st.win, st_np["win"], where)
            check_all(guards, where)
            it += 1
    if B >= 2:
        acc = (flags & ACCEPT) != 0
        assert acc.any() and (active & ~acc).any()                 # both outcomes were in the last batch


def test_whole_image_window():
    """s = H = W: the window is the whole image, vh = vw = 0 for every draw."""
    from nested_diffusion_amd import ops
    B, Cin, H, W = 4, 3, 8, 8
    x, index = make_images(B, Cin, H, W)
    x_best, x_new = ref_init(x, index, EPS, SEED, 0)
    st_np = ref_new_state(B)
    st_np["margin_min"][:] = 1.0
    st_np["win"][:] = -77
    st, guards = guarded_state(st_np)
    gx0, gbest, gnew = Guarded(x), Guarded(x_best), Guarded(x_new)
    for it in range(5):
        ops.square_propose(gx0.t, gbest.t, gnew.t, dev(index), st, 8, it, EPS, SEED, 0)
        ref_propose(x, x_best, x_new, index, st_np["margin_min"], st_np["win"], 8, it, EPS, SEED, 0)
        same("x_new", gnew.t, x_new, f"it={it}")
        assert (st.win.cpu().numpy() == 0).all()
        assert not np.array_equal(x_new[:, :, 0], x_best[:, :, 0]) and not np.array_equal(x_new[:, :, -1], x_best[:, :, -1])
    for g in (gx0, gbest, gnew, *guards.values()):
        g.check("whole-image window")


@pytest.mark.parametrize("s", [1, 5])
def test_window_corners_reach_both_ends(s):
    """200 queries on an 8 x 8 image: the drawn vh and vw reach 0 and H - s / W - s, and every corner and the accumulated x_new match."""
    from nested_diffusion_amd import ops
    B, Cin, H, W = 4, 2, 8, 8
    x, index = make_images(B, Cin, H, W)
    x_best, x_new = ref_init(x, index, EPS, SEED, 0)
    st_np = ref_new_state(B)
    st_np["margin_min"][:] = 1.0
    st, guards = guarded_state(st_np)
    gx0, gbest, gnew = Guarded(x), Guarded(x_best), Guarded(x_new)
    d_index, wins, want_wins = dev(index), [], []
    for it in range(200):
        ops.square_propose(gx0.t, gbest.t, gnew.t, d_index, st, s, it, EPS, SEED, 0)
        wins.append(st.win.clone())
        ref_propose(x, x_best, x_new, index, st_np["margin_min"], st_np["win"], s, it, EPS, SEED, 0)
        want_wins.append(st_np["win"].copy())
    want = np.stack(want_wins)
    same("win", torch.stack(wins), want)
    same("x_new", gnew.t, x_new)
    for b in range(B):
        for k, top in ((0, H - s), (1, W - s)):
            assert want[:, b, k].min() == 0 and want[:, b, k].max() == top, (b, k)
    for g in (gx0, gbest, gnew, *guards.values()):
        g.check("corners")


def test_commit_ignores_a_corner_outside_the_image():
    from nested_diffusion_amd import ops
    B, Cin, H, W, s = 3, 2, 8, 12, 4
    x, index = make_images(B, Cin, H, W)
    x_best, _ = ref_init(x, index, EPS, SEED, 0)
    x_new = np.clip(x_best + f32(0.01), 0, 1).astype(f32)
    st_np = ref_new_state(B)
    st_np["flags"][:] = [ACTIVE | ACCEPT, ACTIVE, ACTIVE | ACCEPT]
    st_np["win"][:] = [[H - s + 1, 0], [0, W - s + 1], [-1, 2]]
    st, guards = guarded_state(st_np)
    gbest, gnew = Guarded(x_best), Guarded(x_new)
    ops.square_commit(gbest.t, gnew.t, st, s)
    same("x_best", gbest.t, x_best)
    same("x_new", gnew.t, x_new)
    gbest.check("x_best")
    gnew.check("x_new")


# ---- keying ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("restart", [0, 3])
def test_a_compacted_subset_draws_what_the_full_batch_draws(restart):
    from nested_diffusion_amd import ops
    B, Cin, H, W, s = 5, 3, 30, 30, 7
    x, index = make_images(B, Cin, H, W)
    keep = np.array([0, 2, 4])
    full_best, full_new = ops.square_init(dev(x), dev(index), EPS, SEED, restart)
    sub_best, sub_new = ops.square_init(dev(x[keep]), dev(index[keep]), EPS, SEED, restart)
    same("stripes", sub_best, full_best[dev(keep)])
    st_f, st_s = ops.SquareState(B, DEV), ops.SquareState(len(keep), DEV)
    st_f.margin_min.fill_(1.0)
    st_s.margin_min.fill_(1.0)
    for it in (0, 1, 17):
        ops.square_propose(dev(x), full_best, full_new, dev(index), st_f, s, it, EPS, SEED, restart)
        ops.square_propose(dev(x[keep]), sub_best, sub_new, dev(index[keep]), st_s, s, it, EPS, SEED, restart)
        same("win", st_s.win, st_f.win[dev(keep)], f"it={it}")
        same("x_new", sub_new, full_new[dev(keep)], f"it={it}")
        for r, b in enumerate(keep):
            assert tuple(st_s.win[r].tolist()) == ref_draw(index[b], it, SEED, restart, H, W, s)[:2]
    # another batch position, the same index: the same draws
    rev_best, _ = ops.square_init(dev(x[keep][::-1].copy()), dev(index[keep][::-1].copy()), EPS, SEED, restart)
    same("stripes, reversed", rev_best.flip(0), full_best[dev(keep)])


# ---- nd_square_accept --------------------------------------------------------------------------------------------------------------------------
def designed_scores(rng, B, C, y, level):
    """Scores in quarters whose margin is exactly level[b]; then the special rows (B >= 16)."""
    sc = (np.round(rng.standard_normal((B, C)) * 4) / 4).astype(f32)
    rows = np.arange(B)
    sc[rows, y] = -np.inf
    other = sc.max(axis=1)
    sc[rows, y] = other + level
    if B >= 16:
        sc[8, y[8]] = np.nan                                       # NaN at the label
        sc[9, (y[9] + 1) % C] = np.nan                             # NaN elsewhere
        sc[10, y[10]] = np.inf                                     # margin +inf
        sc[11, y[11]] = -np.inf                                    # margin -inf: fooled
        sc[12] = np.inf                                            # inf - inf: a NaN margin
        sc[13] = 0.25                                              # every column ties with the label: margin 0, fooled
        sc[14] = -np.inf                                           # -inf - -inf: NaN
    return sc


@pytest.mark.parametrize("C", [2, 3, 1024])
@pytest.mark.parametrize("B", [1, 6, 70])
def test_accept_matches_the_restatement(B, C):
    from nested_diffusion_amd import ops
    rng = np.random.default_rng(B * 2000 + C)
    y = rng.integers(0, C, B)
    y[0] = 0                                                       # a label in the first and in the last column
    if B > 1:
        y[1] = C - 1
    level = (rng.integers(1, 9, B) / 4).astype(f32)                # every row starts active
    if B >= 6:
        level[2:4] = 5.0                                           # still active when the test freezes them by hand
    if B >= 16:
        level[15] = 0.0                                            # a tie between the label and the runner-up at the start: margin 0, frozen
    st_np = ref_new_state(B)
    st, guards = guarded_state(st_np)
    seen = set()
    for it in range(-1, 6):
        if it == 2 and B >= 6:                                     # the two frozen kinds no subtraction of finite scores yields
            for n, v in (("margin_min", [-0.0, np.nan]), ("loss_min", [0.5, 0.25])):
                st_np[n][2:4] = v
                getattr(st, n)[2:4] = dev(np.array(v, f32))
        if it >= 0:
            level = level + (rng.integers(-2, 2, B) / 4).astype(f32)       # -0.5 .. +0.25 per query: new minima, repeats and rises
        sc = designed_scores(rng, B, C, y, level)
        before = {n: st_np[n].copy() for n in ("margin_min", "loss_min", "n_queries")}
        frozen = ~(st_np["margin_min"] > 0) if it >= 0 else np.zeros(B, bool)
        flags = ops.square_accept(dev(sc), dev(y), st, it)
        ref_accept(sc, y, st_np, it)
        where = f"it={it}"
        same("flags", flags, st_np["flags"], where)
        for n in ("margin_min", "loss_min", "n_queries"):
            same(n, getattr(st, n), st_np[n], where)
            same(n + " of the frozen rows", getattr(st, n)[dev(frozen)], before[n][frozen], where)
        assert (st_np["flags"][frozen] == 0).all()
        check_all(guards, where)
        if it >= 0:
            seen |= set(int(v) for v in st_np["flags"])
    assert (st_np["n_queries"] >= 1).all()
    if B >= 6:
        assert seen == {0, ACTIVE, ACTIVE | ACCEPT}
        assert np.signbit(st_np["margin_min"][2]) and np.isnan(st_np["margin_min"][3]) and (st_np["n_queries"][2:4] == 3).all()
    if B >= 16:
        assert st_np["margin_min"][15] == 0 and st_np["n_queries"][15] == 1           # margin 0 counts as fooled: never queried again
        assert st_np["margin_min"][13] == 0 and st_np["margin_min"][11] == -np.inf
        for b in (8, 9, 12, 14):                                   # a NaN margin at the start freezes the row; it never counts as fooled
            assert np.isnan(st_np["margin_min"][b]) and st_np["n_queries"][b] == 1


def test_accept_never_accepts_a_nan_margin_of_an_active_row():
    from nested_diffusion_amd import ops
    B, C = 4, 5
    y = np.array([0, 4, 2, 2])
    st_np = ref_new_state(B)
    st, guards = guarded_state(st_np)
    first = np.tile(np.array([0.0, 0.0, 0.0, 0.0, 0.0], f32), (B, 1))
    first[np.arange(B), y] = 1.0                                   # margin 1 everywhere
    nan_rows = first.copy()
    nan_rows[0, 3] = np.nan
    nan_rows[1, 4] = np.nan
    nan_rows[2] = [5, 5, -9, 5, 5]                                 # margin -14: accepted
    nan_rows[3] = [0, 0, 0.5, 0, 0]                                # margin 0.5: an improvement
    for it, sc in ((-1, first), (0, nan_rows), (1, first)):
        ops.square_accept(dev(sc), dev(y), st, it)
        ref_accept(sc, y, st_np, it)
        for n in ("margin_min", "loss_min", "n_queries", "flags"):
            same(n, getattr(st, n), st_np[n], f"it={it}")
    assert st_np["margin_min"].tolist() == [1.0, 1.0, -14.0, 0.5] and st_np["n_queries"].tolist() == [3, 3, 2, 3]
    check_all(guards, "nan margins")


# ---- the whole loop ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    """{classes: (VisionTransformer, images, the clean predictions)} on 32 x 32 images."""
    from nested_diffusion_amd.mapping import VisionTransformer
    out = {}
    for C in (2, 3):
        vp = ref_cpu.init_vit_params(embed=128, depth=2, patch=16, img=32, num_classes=C, seed=3)
        vit = VisionTransformer(vp, 2, DEV)
        x, _ = make_images(16, 3, 32, 32, seed=C)
        xd = dev(x)
        out[C] = (vit, xd, vit.forward(xd).argmax(dim=1))
    return out


def traced_run(atk, x, y, index, restart=0, oracle=True):
    """attack_single_run with every array and state vector of every query compared against the restatement, fed the GPU's scores.
    Returns the per-query history the state checks need."""
    xn, yn, idx = x.cpu().numpy(), y.cpu().numpy(), index.cpu().numpy()
    B, _, H, W = xn.shape
    ref = dict(st=ref_new_state(B))
    hist = dict(margin_min=[], loss_min=[], flags=[], state=None)

    def trace(i, scores, arrays, st):
        sc = scores.cpu().numpy()
        if oracle:
            if i < 0:
                ref["x_best"], ref["x_new"] = ref_init(xn, idx, atk.eps, atk.seed, restart)
            else:
                s = atk.side(i, H, W)
                ref_propose(xn, ref["x_best"], ref["x_new"], idx, ref["st"]["margin_min"], ref["st"]["win"], s, i, atk.eps, atk.seed, restart)
                # the scores the GPU computed are those of the restatement's candidate: the arrays agreed after the previous query
            ref_accept(sc, yn, ref["st"], i)
            if i >= 0:
                ref_commit(ref["x_best"], ref["x_new"], ref["st"]["win"], ref["st"]["flags"], s)
            where = f"query {i}"
            same("x_best", arrays["x_best"], ref["x_best"], where)
            same("x_new", arrays["x_new"], ref["x_new"], where)
            for n in ("margin_min", "loss_min", "n_queries", "flags"):
                same(n, getattr(st, n), ref["st"][n], where)
            if i >= 0:
                act = (ref["st"]["flags"] & ACTIVE) != 0
                same("win", st.win[dev(act)], ref["st"]["win"][act], where)
        assert torch.equal(arrays["x_new"], arrays["x_best"]), f"query {i}"
        hist["margin_min"].append(st.margin_min.cpu().numpy().copy())
        hist["loss_min"].append(st.loss_min.cpu().numpy().copy())
        hist["flags"].append(st.flags.cpu().numpy().copy())
        hist["state"] = st

    n_q, x_best = atk.attack_single_run(x, y, index, restart=restart, trace=trace)
    return n_q, x_best, hist


@pytest.mark.parametrize("C", [2, 3])
def test_whole_loop_matches_the_restatement(tiny, C):
    from nested_diffusion_amd.square import SquareAttack
    vit, x, pred = tiny[C]
    B, n_queries = 6, 300
    x, y = x[:B].contiguous(), pred[:B].contiguous()
    index = torch.arange(B, device=DEV) * 5 + (1 << 31)
    atk = SquareAttack(vit, eps=EPS, n_queries=n_queries, seed=SEED, check_every=0)
    n_q, x_best, hist = traced_run(atk, x, y, index)
    assert len(hist["flags"]) == n_queries + 1
    xb, xn = x_best.cpu().numpy(), x.cpu().numpy()
    e = f32(EPS)
    assert xb.min() >= 0.0 and xb.max() <= 1.0
    assert (xb >= xn - e).all() and (xb <= xn + e).all()           # elementwise within the fp32 values x0 - eps and x0 + eps
    mm, lm = np.stack(hist["margin_min"]), np.stack(hist["loss_min"])
    assert (lm[1:] <= lm[:-1]).all()                               # loss_min never rises
    active = mm[:-1] > 0                                           # row b was active in query i iff margin_min > 0 before it
    same("n_queries", n_q, (1 + active.sum(axis=0)).astype(np.int32))
    flags = np.stack(hist["flags"])[1:]
    assert ((flags & ACTIVE) != 0).sum() == active.sum() and ((flags == ACTIVE | ACCEPT).any() and (flags == ACTIVE).any())
    # early exit: asking after every query whether a row is still active changes no bit of the result
    st0 = hist["state"]
    keep = {}
    atk1 = SquareAttack(vit, eps=EPS, n_queries=n_queries, seed=SEED, check_every=1)
    n_q1, x_best1 = atk1.attack_single_run(x, y, index, trace=lambda i, sc, arrays, st: keep.update(st=st))
    same("x_best, check_every=1", x_best1, x_best)
    same("n_queries, check_every=1", n_q1, n_q)
    for n in ("margin_min", "loss_min"):
        same(n + ", check_every=1", getattr(keep["st"], n), getattr(st0, n))


def test_early_exit_stops_querying(tiny):
    """Every row is misclassified from the start: with the check the loop stops before its first query, without it it runs them all (on
    frozen rows: nothing changes); the results are equal bit for bit."""
    from nested_diffusion_amd.square import SquareAttack
    vit, x, pred = tiny[2]
    x, y = x[:4].contiguous(), (1 - pred[:4]).contiguous()
    index = torch.arange(4, device=DEV)
    calls = []

    def predict(t):
        calls.append(1)
        return vit.forward(t)

    out = {}
    for every in (1, 0):
        calls.clear()
        keep = {}
        atk = SquareAttack(predict, eps=1e-4, n_queries=20, seed=1, check_every=every, device=DEV)
        n_q, x_best = atk.attack_single_run(x, y, index, trace=lambda i, sc, arrays, st: keep.update(st=st, x_new=arrays["x_new"]))
        out[every] = (n_q.clone(), x_best.clone(), keep["st"].margin_min.clone(), keep["st"].loss_min.clone(), keep["x_new"].clone())
        assert len(calls) == (1 if every else 21)
        assert (n_q == 1).all() and bool((keep["st"].margin_min <= 0).all())
    for a, b in zip(out[1], out[0]):
        same("early exit", a, b)
    same("x_new", out[0][4], out[0][1])


def test_callable_predict_and_perturb_row_rules(tiny):
    from nested_diffusion_amd.square import SquareAttack
    vit, x, pred = tiny[3]
    B = 8
    x, y = x[:B].contiguous(), pred[:B].contiguous()
    index = torch.arange(B, device=DEV) + 50
    runs = {}
    for name, predict in (("vit", vit), ("callable", lambda t: 0.5 * vit.forward(t))):
        atk = SquareAttack(predict, eps=EPS, n_queries=60, seed=SEED, check_every=0, device=DEV)
        n_q, x_best, hist = traced_run(atk, x, y, index, oracle=(name == "callable"))
        runs[name] = (np.stack(hist["flags"]), n_q.cpu().numpy(), x_best)
    assert (runs["vit"][0] == runs["callable"][0]).all()           # halving the scores halves every margin exactly: the same decisions
    assert (runs["vit"][1] == runs["callable"][1]).all() and torch.equal(runs["vit"][2], runs["callable"][2])

    # perturb: rows the clean model misclassifies, and rows no restart fools, come back unchanged
    y_mixed = y.clone()
    y_mixed[:3] = (y[:3] + 1) % 3                                  # three rows the clean model misclassifies
    for eps, restarts in ((EPS, 2), (1e-6, 1)):
        atk = SquareAttack(lambda t: 0.5 * vit.forward(t), eps=eps, n_queries=40, n_restarts=restarts, seed=3, device=DEV)
        adv = atk.perturb(x, y_mixed, index=index)
        fooled = vit.forward(adv).argmax(dim=1) != y_mixed
        changed = (adv != x).flatten(1).any(dim=1)
        assert not bool(changed[:3].any())                         # misclassified from the start: not attacked
        assert bool((changed[3:] == fooled[3:]).all())             # a row is replaced iff the attack fooled the model on it
        assert float((adv - x).abs().max()) <= eps + 2.0 ** -23 and float(adv.min()) >= 0.0 and float(adv.max()) <= 1.0
        adv2, success = atk.generate_attack(x, y_mixed, first_image=50)
        assert torch.equal(adv2, adv) and torch.equal(success, fooled)
    assert not bool(changed.any())                                 # eps = 1e-6 fools nothing here: the whole batch comes back unchanged
    with pytest.raises(ValueError, match=r"labels must lie in \[0, 3\)"):
        atk.perturb(x, torch.full((B,), 3, device=DEV))


def test_strength(tiny):
    """eps = 0.3, 500 queries, B = 16 on the tiny ViT with its own predictions as labels.  Asserted: at least as many rows are fooled as
    the stripe start alone fools, and the summed loss_min ends strictly below its value after the start.  Printed, not asserted: the
    robust accuracy reached (measured on the MI355X: the stripes fool 2 of 16, the loop 16 of 16 after a mean of 20.5 queries: robust
    accuracy 0.0; sum of loss_min 14.27 -> -2.59)."""
    from nested_diffusion_amd.square import SquareAttack
    vit, x, pred = tiny[2]
    B = 16
    index = torch.arange(B, device=DEV)
    seen = {}

    def trace(i, scores, arrays, st):
        if i < 0:
            seen["start_fooled"] = int((st.margin_min <= 0).sum())
            seen["start_loss"] = float(st.loss_min.double().sum())
        seen["st"] = st

    atk = SquareAttack(vit, eps=0.3, n_queries=500, seed=0)
    n_q, x_best = atk.attack_single_run(x, pred, index, trace=trace)
    st = seen["st"]
    fooled = int((st.margin_min <= 0).sum())
    end_loss = float(st.loss_min.double().sum())
    still = vit.forward(x_best).argmax(dim=1) == pred
    print(f"square strength: stripes fool {seen['start_fooled']}/{B}, after 500 queries {fooled}/{B}; robust accuracy {float(still.float().mean()):.4f}; "
          f"sum loss_min {seen['start_loss']:.4f} -> {end_loss:.4f}; mean queries {float(n_q.float().mean()):.1f}")
    assert fooled >= seen["start_fooled"]
    assert end_loss < seen["start_loss"]
    assert int((~still).sum()) >= fooled - int((st.margin_min == 0).sum())     # a fooled row's x_best is misclassified (a tie may go either way)


# ---- through the runner ------------------------------------------------------------------------------------------------------------------------
def test_test_atk_takes_a_square_attack(tmp_path, monkeypatch, capsys):
    """Diffusion.test_atk(attack=SquareAttack(...)) end to end at the smallest configuration of tests/test_gpu_attack_e2e.py: its report
    equals test_atk on apply_attack's output, and make_attacks.write_attacked_set writes a Test_attacks_SQUARE tree."""
    import yaml
    import nested_diffusion_amd.runner as runner_mod
    from nested_diffusion_amd import main as nd_main
    from nested_diffusion_amd import make_attacks
    from nested_diffusion_amd.attack import apply_attack
    from nested_diffusion_amd.data import ImageFolderDataset
    from nested_diffusion_amd.square import SquareAttack
    from test_gpu_attack_e2e import FLAGS, _reload_png, _run_main
    from test_gpu_cli import _write_image_tree, _write_run
    tmp = str(tmp_path)
    ypath, *_ = _write_run(tmp, T=6, K=5, B=3, img=224)
    dataroot = os.path.join(tmp, "data")
    _write_image_tree(dataroot)
    clean = ImageFolderDataset(os.path.join(dataroot, "testing"), "ChestXRay", "grayscaled")
    items = [clean[i] for i in range(3)]
    batches = [(torch.stack([x for x, _ in items]), torch.tensor([t for _, t in items]))]
    eps = 8 / 255
    reports = {}
    orig_atk = runner_mod.Diffusion.test_atk

    def spy(self, test_loader=None, attack=None):
        atk = SquareAttack(self.cond_pred_model, eps=eps, n_queries=20, seed=3)
        assert atk.model is self.cond_pred_model.vit
        orig_atk(self, test_loader=batches, attack=atk)
        reports["square"] = self.last_report
        adv = [(apply_attack(atk, x.to(self.device), t.to(self.device), "SQUARE", first_image=3 * n).cpu(), t) for n, (x, t) in enumerate(batches)]
        reports["max"] = max(float((a - x).abs().max()) for (a, _), (x, _) in zip(adv, batches))
        orig_atk(self, test_loader=adv)
        reports["apply"] = self.last_report
        return orig_atk(self, test_loader=batches)

    monkeypatch.setattr(runner_mod.Diffusion, "test_atk", spy)
    assert _run_main(FLAGS + ["--config", ypath, "--dataroot", dataroot, "--doc", "sq", "--exp", os.path.join(tmp, "r")]) == 0
    a, b = reports["square"], reports["apply"]
    for k in a:
        assert torch.allclose(torch.as_tensor(a[k]), torch.as_tensor(b[k]), rtol=0, atol=0, equal_nan=True), k
    assert reports["max"] <= eps + 2.0 ** -23                      # eps and half an ulp of the sum x + eps
    # the attacked tree
    with open(ypath) as f:
        config = nd_main.dict2namespace(yaml.safe_load(f))
    device = torch.device("cuda", 0)
    out = os.path.join(tmp, "attacked")
    atk = SquareAttack(make_attacks.load_vit(config, device), eps=eps, n_queries=20, seed=3)
    make_attacks.write_attacked_set(config, atk, "SQUARE", out, batch_size=3, dataroot=dataroot)
    tree = os.path.join(out, "Test_attacks_SQUARE")
    assert sorted(os.listdir(tree)) == ["NORMAL", "PNEUMONIA"]
    n = 0
    for path, target in clean.samples:
        cls = os.path.basename(os.path.dirname(path))
        stem = os.path.splitext(os.path.basename(path))[0]
        adv = _reload_png(os.path.join(tree, cls, stem + ".png"))
        x, _ = clean[clean.samples.index((path, target))]
        assert float((adv - x).abs().max()) <= eps + 0.5 / 255 + 1e-6
        n += 1
    assert n == 7
