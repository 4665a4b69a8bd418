"""The L2 Square attack on the GPU (nd_square_l2_* in csrc/nd_square_l2.hip, square.SquareL2Attack, autoattack.WorstCase): every sum a
kernel reports against the float64 sum of the same fp32 terms, and, given the kernel's own sums, every array bit for bit (the int32 view of
the floats) against the per-kernel numpy restatement of tests/test_square_l2_host.py, which that file checks against an independently
written whole-array version on the CPU.  Every array a kernel writes lies inside a larger buffer with sentinels in front of and behind it,
at an address that is not 16-byte aligned; the sentinels are checked after every call.  The same calls on torch's own (aligned)
allocations take the 16-byte path where W % 4 == 0 and must give the same bits.

The bound of a sum: any summation order of n non-negative fp32 terms has at most n - 1 additions of two non-zero numbers, each with a
relative error of at most 2^-24 on a partial sum that never exceeds the total, so |sum - exact| <= (n + 1) * 2^-24 * exact (the bound
tests/test_gpu_apgd_l2.py derives); adding a masked-out 0 is exact."""
import os

import numpy as np
import pytest
import torch

from oracle import ref_cpu
from test_gpu_square import Guarded, check_all, dev, make_images, margins
from test_square_host import ACCEPT, ACTIVE, ref_accept, same
from test_square_l2_host import (S_ALL, S_MASK, S_NEW, S_OUT, S_U, S_W1, ref_l2_commit, ref_l2_draw, ref_l2_init, ref_l2_new_state,
                                 ref_l2_propose)

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32
U = 2.0 ** -24
EPS = 0.5
SEED = (9 << 32) | 1234
# one 5 x 5 image of one channel (s0 = 1), 8 x 8, a non-square image, rows that are not 16-byte aligned (W = 30), more than 64 images
SHAPES = [(1, 1, 5, 5), (4, 3, 8, 8), (3, 3, 32, 48), (5, 3, 30, 30), (70, 3, 32, 32)]
NAMES = {S_W1: "S_w1", S_ALL: "S_all", S_MASK: "S_mask", S_OUT: "S_out", S_U: "S_u", S_NEW: "S_new"}
POISON = f32(-7.25)


# ---- helpers --------------------------------------------------------------------------------------------------------------------------
def attack(**kw):
    from nested_diffusion_amd.square import SquareL2Attack
    kw.setdefault("eps", EPS)
    return SquareL2Attack(kw.pop("predict", lambda x: None), **kw)


ETA = attack()


def eta_np(s):
    return ETA.eta(s).numpy()


def sides_of(shape):
    m = min(shape[2], shape[3])
    return sorted({3, 5, 7, m - 1 + m % 2} & set(range(3, m + 1)))


def guarded_l2_state(st_np, Cin, H, W):
    """An ops.SquareL2State whose arrays are Guarded copies of the dict st_np (and a Guarded workspace); returns (state, guards)."""
    from nested_diffusion_amd import ops
    B = st_np["flags"].shape[0]
    st = ops.SquareL2State(B, Cin, H, W, DEV)
    guards = {n: Guarded(st_np[n]) for n in ("margin_min", "loss_min", "n_queries", "flags", "win", "sums")}
    guards["ws"] = Guarded(np.full(st.ws.numel(), 1e30, f32))     # stale partials must never be read before they are written
    for n, g in guards.items():
        setattr(st, n, g.t)
    return st, guards


def check_sum(name, got, terms, where):
    """|got - exact| <= (terms + 1) * 2^-24 * exact, exact the float64 sum of the fp32 terms."""
    exact = float(np.asarray(terms, dtype=np.float64).sum())
    bound = (len(terms) + 1) * U * exact
    assert abs(float(got) - exact) <= bound, f"{where}: {name} = {float(got)!r}, float64 sum {exact!r}, |difference| {abs(float(got) - exact):.3e} > {bound:.3e}"


def check_sums(sums, terms, active, where):
    """The six sums of every active row, and S_mask + S_out against S_all."""
    for b in np.flatnonzero(active):
        for k, name in NAMES.items():
            check_sum(name, sums[k, b], terms[b][k], f"{where} row {b}")
        n, s_all = len(terms[b][S_ALL]), float(sums[S_ALL, b])
        assert abs(float(sums[S_MASK, b]) + float(sums[S_OUT, b]) - s_all) <= (n + 1) * U * s_all, (where, b, sums[:, b])


def start(shape, restart=0, seed=0):
    """x0, index and the restatement's start for `shape`."""
    x, index = make_images(*shape, seed=seed)
    x_best, x_new, _ = ref_l2_init(x, index, eta_np(min(shape[2:]) // 5), EPS, SEED, restart)
    return x, index, x_best, x_new


def gpu_propose(x, x_best, x_new, index, st_np, s, it, restart=0, eps=EPS, guarded=True):
    """One nd_square_l2_propose on device copies (guarded and misaligned, or torch's own allocations); returns x_new, win and sums as
    numpy, after checking the sentinels and that x0 and x_best were only read."""
    from nested_diffusion_amd import ops
    B, Cin, H, W = x.shape
    if guarded:
        st, guards = guarded_l2_state(st_np, Cin, H, W)
        gx0, gbest, gnew, geta = Guarded(x), Guarded(x_best), Guarded(x_new), Guarded(eta_np(s))
        guards.update(x0=gx0, x_best=gbest, x_new=gnew, eta=geta)
        ops.square_l2_propose(gx0.t, gbest.t, gnew.t, dev(index), st, geta.t, s, it, eps, SEED, restart)
        check_all(guards, f"propose s={s} it={it}")
        same("x0", gx0.t, x)
        same("x_best", gbest.t, x_best)
        same("margin_min", st.margin_min, st_np["margin_min"])
        out = gnew.t
    else:
        st = ops.SquareL2State(B, Cin, H, W, DEV)
        for n in ("margin_min", "win", "sums"):
            getattr(st, n).copy_(dev(st_np[n]))
        out = dev(x_new)
        ops.square_l2_propose(dev(x), dev(x_best), out, dev(index), st, ETA.eta(s, DEV), s, it, eps, SEED, restart)
    return out.cpu().numpy(), st.win.cpu().numpy(), st.sums.cpu().numpy()


# ---- nd_square_l2_init ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("restart", [0, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_init_matches_the_restatement(shape, restart):
    from nested_diffusion_amd import _lib, ops
    B, Cin, H, W = shape
    x, index = make_images(*shape)
    s0 = min(H, W) // 5
    eta0 = eta_np(s0)
    x_best, x_new, sums = ops.square_l2_init(dev(x), dev(index), ETA.eta(s0, DEV), EPS, SEED, restart)
    terms = []
    want_best, want_new, _ = ref_l2_init(x, index, eta0, EPS, SEED, restart, sums=sums.cpu().numpy(), terms=terms)
    for b in range(B):
        check_sum("sum D0^2", sums[b], terms[b], f"init row {b}")
    same("x_best", x_best, want_best)
    same("x_new", x_new, want_new)
    d = (want_best.astype(np.float64) - x).reshape(B, -1)
    assert (np.sqrt((d ** 2).sum(1)) <= EPS * (1 + (Cin * H * W + 8) * U)).all() and (d > 0).any() and (d < 0).any()
    # through guarded, misaligned arrays: the same bits (sums included), and nothing outside the arrays is touched
    gx, ge, gb, gn = Guarded(x), Guarded(eta0), Guarded(np.zeros_like(x)), Guarded(np.zeros_like(x))
    gs, gw = Guarded(np.zeros(B, f32)), Guarded(np.full(B * ops.square_l2_ws_floats(Cin, H, W), 1e30, f32))
    d_index = dev(index)
    _lib.check(_lib.load().nd_square_l2_init(gx.t.data_ptr(), d_index.data_ptr(), ge.t.data_ptr(), gb.t.data_ptr(), gn.t.data_ptr(),
                                             gs.t.data_ptr(), gw.t.data_ptr(), B, Cin, H, W, s0, SEED, restart, EPS, 0.0, 1.0,
                                             torch.cuda.current_stream().cuda_stream), "nd_square_l2_init")
    torch.cuda.synchronize()
    same("sums (guarded)", gs.t, sums)
    same("x_best (guarded)", gb.t, want_best)
    same("x_new (guarded)", gn.t, want_new)
    for g in (gx, ge, gb, gn, gs, gw):
        g.check("init")
    if restart:
        assert not np.array_equal(want_best, ref_l2_init(x, index, eta0, EPS, SEED, 0)[0])      # a restart draws other signs


# ---- nd_square_l2_propose and nd_square_l2_commit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_propose_and_commit_match_the_restatement(shape):
    """Two queries per side on one pair of arrays, accepts and rejects mixed in the batch, frozen rows of every kind among them: after
    every launch the sums against float64, every array against the restatement given those sums, the frozen rows against their bits
    before the launch; then the same call on aligned allocations gives the same bits."""
    from nested_diffusion_amd import ops
    B, Cin, H, W = shape
    restart = 1
    x, index, x_best, x_new = start(shape, restart)
    st_np = ref_l2_new_state(B)
    st_np["margin_min"] = margins(B)
    st_np["win"][:] = -77                                          # a frozen row's corners and sums are never written
    st_np["sums"][:] = POISON
    active = st_np["margin_min"] > 0
    x_new[~active] = POISON                                        # ... nor is its image
    it = 0
    for s in sides_of(shape):
        for _ in range(2):
            where = f"propose s={s} it={it}"
            before_new, before = x_new.copy(), {n: st_np[n].copy() for n in ("win", "sums")}
            got_new, got_win, got_sums = gpu_propose(x, x_best, x_new, index, st_np, s, it, restart)
            terms = {}
            st_np["sums"][:] = got_sums
            ref_l2_propose(x, x_best, x_new, index, st_np["margin_min"], eta_np(s), st_np["win"], st_np["sums"], s, it, EPS, SEED, restart,
                           given=True, terms=terms)
            check_sums(got_sums, terms, active, where)
            same("x_new", got_new, x_new, where)
            same("win", got_win, st_np["win"], where)
            same("x_new of the frozen rows", got_new[~active], before_new[~active], where)
            same("win of the frozen rows", got_win[~active], before["win"][~active], where)
            same("sums of the frozen rows", got_sums[:, ~active], before["sums"][:, ~active], where)
            assert (got_win[active, 0::2] <= H - s).all() and (got_win[active, 1::2] <= W - s).all() and (got_win[active] >= 0).all()
            # torch's own allocations: the 16-byte path where W % 4 == 0
            al_new, al_win, al_sums = gpu_propose(x, x_best, before_new, index, dict(st_np, **before), s, it, restart, guarded=False)
            same("x_new (aligned)", al_new, got_new, where)
            same("win (aligned)", al_win, got_win, where)
            same("sums (aligned)", al_sums, got_sums, where)
            # the commit: accepts and rejects mixed; a frozen row with stale flag bits would be a caller's error and is not produced
            flags = np.where(active, ACTIVE | np.where((np.arange(B) + it) % 2 == 0, ACCEPT, 0), 0).astype(np.int32)
            st_np["flags"][:] = flags
            st, guards = guarded_l2_state(st_np, Cin, H, W)
            gbest, gnew = Guarded(x_best), Guarded(x_new)
            before_best = x_best.copy()
            ops.square_l2_commit(gbest.t, gnew.t, st)
            ref_l2_commit(x_best, x_new, flags)
            where = f"commit s={s} it={it}"
            same("x_best", gbest.t, x_best, where)
            same("x_new", gnew.t, x_new, where)
            acc = (flags & ACCEPT) != 0
            same("x_best of the accepted rows", gbest.t[dev(acc)], x_new[acc], where)
            same("x_best of the other rows", gbest.t[dev(~acc)], before_best[~acc], where)
            check_all(dict(guards, x_best=gbest, x_new=gnew), where)
            it += 1


def test_commit_copies_accepted_rows_only():
    """Every flag value, on aligned and on misaligned arrays, on an image whose size is not a multiple of 4."""
    from nested_diffusion_amd import ops
    for shape in ((6, 3, 5, 5), (6, 3, 8, 8)):
        B, Cin, H, W = shape
        rng = np.random.default_rng(B * H)
        x_best, x_new = rng.random(shape, dtype=f32), rng.random(shape, dtype=f32)
        flags = np.array([ACTIVE | ACCEPT, ACTIVE, 0, ACCEPT, ACTIVE | ACCEPT, 0], np.int32)        # ACCEPT without ACTIVE copies nothing
        want = x_best.copy()
        ref_l2_commit(want, x_new, flags)
        assert np.array_equal(want[0], x_new[0]) and np.array_equal(want[3], x_best[3])
        st_np = ref_l2_new_state(B)
        st_np["flags"][:] = flags
        st, guards = guarded_l2_state(st_np, Cin, H, W)
        gbest, gnew = Guarded(x_best), Guarded(x_new)
        ops.square_l2_commit(gbest.t, gnew.t, st)
        same("x_best", gbest.t, want)
        same("x_new", gnew.t, x_new)
        check_all(dict(guards, x_best=gbest, x_new=gnew), "commit")
        d_best, d_new = dev(x_best), dev(x_new)
        st.flags = dev(flags)
        ops.square_l2_commit(d_best, d_new, st)
        same("x_best (aligned)", d_best, want)
        same("x_new (aligned)", d_new, x_new)


def test_a_row_has_the_same_bits_alone_in_the_batch_and_in_a_subset():
    shape = (70, 3, 32, 32)
    B, Cin, H, W = shape
    x, index, x_best, x_new = start(shape)
    st_np = ref_l2_new_state(B)
    st_np["margin_min"][:] = 1.0
    for s, it in ((7, 0), (31, 5)):
        full = gpu_propose(x, x_best, x_new, index, st_np, s, it)
        for rows in ([3, 17, 69], [17], [69]):
            sub = ref_l2_new_state(len(rows))
            sub["margin_min"][:] = 1.0
            for guarded in (True, False):
                got = gpu_propose(x[rows], x_best[rows], x_new[rows], index[rows], sub, s, it, guarded=guarded)
                same("x_new", got[0], full[0][rows], f"rows {rows}")
                same("win", got[1], full[1][rows], f"rows {rows}")
                same("sums", got[2], full[2][:, rows], f"rows {rows}")


def test_window_cases_and_degenerate_perturbations():
    """On 8 x 8 images, queries the host restatement selects: w1 = w2, partial overlap, disjoint windows, w1 at (H - s, W - s), s = 7 (the
    largest odd side); in each, row 0 is a general point, row 1 has D = 0 on w1, row 2 has x_best = x0 everywhere and row 3 has
    ||x_best - x0|| > eps (the max(., 0) branch).  x0 holds exact 0.0 and 1.0."""
    B, Cin, H, W = 4, 3, 8, 8
    x, index, x_best0, _ = start((B, Cin, H, W))
    index[:] = 12345                                               # one image index: the four rows draw the same windows
    assert (x == 0.0).any() and (x == 1.0).any()
    found = {}
    for s in (3, 5, 7):
        for it in range(400):
            vh1, vw1, vh2, vw2, _, _ = ref_l2_draw(12345, it, SEED, 0, H, W, s)
            dh, dw = abs(vh1 - vh2), abs(vw1 - vw2)
            kind = "same" if (dh, dw) == (0, 0) else "partial" if dh < s and dw < s else "disjoint"
            found.setdefault((kind, s), it)
            if (vh1, vw1) == (H - s, W - s):
                found.setdefault(("corner", s), it)
    cases = [("same", 7), ("same", 5), ("partial", 3), ("partial", 7), ("disjoint", 3), ("corner", 3), ("corner", 5), ("corner", 7)]
    assert all(c in found for c in cases), sorted(found)
    st_np = ref_l2_new_state(B)
    st_np["margin_min"][:] = 1.0
    for kind, s in cases:
        it = found[(kind, s)]
        vh1, vw1, vh2, vw2, _, _ = ref_l2_draw(12345, it, SEED, 0, H, W, s)
        x_best = x_best0.copy()
        x_best[1, :, vh1:vh1 + s, vw1:vw1 + s] = x[1, :, vh1:vh1 + s, vw1:vw1 + s]
        x_best[2] = x[2]
        x_best[3] = np.clip(x[3] + np.where(x[3] < 0.5, f32(0.25), f32(-0.25)), 0, 1).astype(f32)
        assert np.sqrt(((x_best[3].astype(np.float64) - x[3]) ** 2).sum()) > EPS
        where = f"{kind} s={s} it={it}"
        got_new, got_win, got_sums = gpu_propose(x, x_best, np.full_like(x, POISON), index, st_np, s, it)
        x_new, terms, ref = np.full_like(x, POISON), {}, ref_l2_new_state(B)
        ref["sums"][:] = got_sums
        ref_l2_propose(x, x_best, x_new, index, st_np["margin_min"], eta_np(s), ref["win"], ref["sums"], s, it, EPS, SEED, given=True, terms=terms)
        assert ref["win"][0].tolist() == [vh1, vw1, vh2, vw2]
        assert got_sums[S_W1, 1] == 0 and (got_sums[:4, 2] == 0).all() and got_sums[S_U, 2] > 0, where
        assert float(np.sqrt(got_sums[S_ALL, 3])) > EPS, where
        if kind == "same":
            same("S_mask = S_w1", got_sums[S_MASK], got_sums[S_W1], where)
        for b in range(B):
            for k, name in NAMES.items():
                if float(np.asarray(terms[b][k], np.float64).sum()) == 0.0:
                    assert got_sums[k, b] == 0, (where, b, name)
        check_sums(got_sums, terms, np.ones(B, bool), where)
        same("x_new", got_new, x_new, where)
        same("win", got_win, ref["win"], where)
        assert np.isfinite(got_new).all() and got_new.min() >= 0.0 and got_new.max() <= 1.0
        d = (got_new.astype(np.float64) - x).reshape(B, -1)
        assert (np.sqrt((d ** 2).sum(1)) <= EPS * (1 + (Cin * H * W + 8) * U) + np.sqrt(Cin * H * W) * U).all(), where


@pytest.mark.parametrize("s", [201, 9])
def test_production_image_geometry(s):
    """3 x 224 x 224: 168 partials per image in the whole-image passes, 151 (s = 201) or 7 (s = 9) in the window passes; rows of 56 quads
    (lanes 56 .. 63 idle) and window rows longer than a wave."""
    shape = (2, 3, 224, 224)
    B, Cin, H, W = shape
    x, index, x_best, x_new = start(shape, seed=s)
    st_np = ref_l2_new_state(B)
    st_np["margin_min"][:] = (1.0, 0.25)
    got_new, got_win, got_sums = gpu_propose(x, x_best, x_new, index, st_np, s, 3)
    terms, ref = {}, ref_l2_new_state(B)
    ref["sums"][:] = got_sums
    ref_l2_propose(x, x_best, x_new, index, st_np["margin_min"], eta_np(s), ref["win"], ref["sums"], s, 3, EPS, SEED, given=True, terms=terms)
    check_sums(got_sums, terms, np.ones(B, bool), f"s={s}")
    same("x_new", got_new, x_new)
    same("win", got_win, ref["win"])
    al = gpu_propose(x, x_best, x_new, index, st_np, s, 3, guarded=False)
    same("x_new (aligned)", al[0], got_new)
    same("sums (aligned)", al[2], got_sums)


def test_init_at_the_production_image():
    from nested_diffusion_amd import ops
    shape = (2, 3, 224, 224)
    x, index = make_images(*shape)
    x_best, x_new, sums = ops.square_l2_init(dev(x), dev(index), ETA.eta(44, DEV), EPS, SEED, 0)
    terms = []
    want_best, _, _ = ref_l2_init(x, index, eta_np(44), EPS, SEED, 0, sums=sums.cpu().numpy(), terms=terms)
    for b in range(2):
        check_sum("sum D0^2", sums[b], terms[b], f"init row {b}")
    same("x_best", x_best, want_best)
    same("x_new", x_new, want_best)
    assert (want_best[:, :, :2] == x[:, :, :2]).all() and (want_best[:, :, :, -2:] == x[:, :, :, -2:]).all()       # 224 - 5 * 44 = 4: margins of 2


# ---- the whole loop ----------------------------------------------------------------------------------------------------------------------------
def traced_run(atk, x, y, index, restart=0):
    """attack_single_run with every array and state vector of every query compared against the restatement, fed the GPU's scores and
    sums.  Returns the per-query history."""
    xn, yn, idx = x.cpu().numpy(), y.cpu().numpy(), index.cpu().numpy()
    B, Cin, H, W = xn.shape
    ref = dict(st=ref_l2_new_state(B))
    hist = dict(margin_min=[], loss_min=[], flags=[], x_best=[], state=None)

    def trace(i, scores, arrays, st):
        sc = scores.cpu().numpy()
        where = f"query {i}"
        if i < 0:
            ref["x_best"], ref["x_new"], _ = ref_l2_init(xn, idx, eta_np(min(H, W) // 5), atk.eps, atk.seed, restart,
                                                         sums=arrays["init_sums"].cpu().numpy())
        else:
            s = atk.side(i, H, W)
            ref["st"]["sums"][:] = st.sums.cpu().numpy()
            ref_l2_propose(xn, ref["x_best"], ref["x_new"], idx, ref["st"]["margin_min"], eta_np(s), ref["st"]["win"], ref["st"]["sums"], s, i,
                           atk.eps, atk.seed, restart, given=True)
        ref_accept(sc, yn, ref["st"], i)
        if i >= 0:
            ref_l2_commit(ref["x_best"], ref["x_new"], ref["st"]["flags"])
            act = (ref["st"]["flags"] & ACTIVE) != 0
            same("win", st.win[dev(act)], ref["st"]["win"][act], where)
        same("x_best", arrays["x_best"], ref["x_best"], where)
        same("x_new", arrays["x_new"], ref["x_new"], where)
        for n in ("margin_min", "loss_min", "n_queries", "flags"):
            same(n, getattr(st, n), ref["st"][n], where)
        for n in ("margin_min", "loss_min", "flags"):
            hist[n].append(ref["st"][n].copy())
        hist["state"] = st

    n_q, x_best = atk.attack_single_run(x, y, index, restart=restart, trace=trace)
    return n_q, x_best, hist


def linear_model(seed=7, n=3 * 16 * 16):
    """x.flatten(1) @ w with w[:, 1] = -w[:, 0] and sum w[:, 0] = 0: the margins of uniform images are centred on 0 with a spread of
    about 16 * 0.1, and eps = 0.5 can move one by at most 2 * 0.5 * ||w[:, 0]|| ~ 2.8, so some rows are fooled and some are not."""
    w0 = torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 0.1
    w0 -= w0.mean()
    w = torch.stack([w0, -w0], dim=1).contiguous().to(DEV)
    return lambda t: t.flatten(1) @ w


def test_whole_loop_on_a_linear_model():
    B, Cin, H, W, eps, n_queries = 6, 3, 16, 16, 0.5, 60
    model = linear_model()
    x = torch.rand(B, Cin, H, W, generator=torch.Generator().manual_seed(5)).to(DEV)
    clean = model(x)
    y = clean.argmax(dim=1)
    clean_margin = (clean.gather(1, y[:, None]) - clean.gather(1, 1 - y[:, None])).flatten().cpu().numpy()
    index = torch.arange(B, device=DEV) * 5 + (1 << 31)
    atk = attack(predict=model, eps=eps, n_queries=n_queries, seed=SEED, check_every=0, device=DEV)
    n_q, x_best, hist = traced_run(atk, x, y, index)
    assert len(hist["flags"]) == n_queries + 1
    mm, lm = np.stack(hist["margin_min"]), np.stack(hist["loss_min"])
    assert (lm[1:] <= lm[:-1]).all()                               # loss_min never rises
    active = mm[:-1] > 0                                           # row b was active in query i iff margin_min > 0 before it
    same("n_queries", n_q, (1 + active.sum(axis=0)).astype(np.int32))
    flags = np.stack(hist["flags"])[1:]
    assert ((flags & ACTIVE) != 0).sum() == active.sum() and (flags == ACTIVE | ACCEPT).any() and (flags == ACTIVE).any()
    n = Cin * H * W
    dist = (x_best.double() - x.double()).flatten(1).norm(dim=1).cpu().numpy()
    assert (dist <= eps * (1 + (n + 8) * U) + np.sqrt(n) * U).all(), dist
    assert float(x_best.min()) >= 0 and float(x_best.max()) <= 1
    fell = lm[-1] < clean_margin
    print(f"square l2 linear model: clean margins {clean_margin}, final loss_min {lm[-1]}, ||x_best - x0|| {dist}, queries {n_q.tolist()}")
    assert fell.sum() * 2 >= B, (clean_margin, lm[-1])
    # perturb: rows misclassified at the start come back unchanged, fooled rows are replaced, the rest come back unchanged
    y_mixed = y.clone()
    y_mixed[[1, 4]] = 1 - y[[1, 4]]
    adv = attack(predict=model, eps=eps, n_queries=n_queries, seed=SEED, device=DEV).perturb(x, y_mixed, index=index)
    changed = (adv != x).flatten(1).any(dim=1)
    fooled = model(adv).argmax(dim=1) != y_mixed
    assert not bool(changed[[1, 4]].any()) and bool((changed == (fooled & (y_mixed == y))).all())
    with pytest.raises(ValueError, match="at least 5 x 5"):
        attack(predict=model, device=DEV).perturb(torch.zeros(2, 3, 4, 4, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV))


# ---- integration ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    """The small ViT of tests/test_gpu_apgd_l2.py."""
    from nested_diffusion_amd.mapping import VisionTransformer
    return VisionTransformer(ref_cpu.init_vit_params(embed=128, depth=5, patch=16, img=32, seed=3), 2, DEV)


def graded_images():
    from test_gpu_attack import images
    return (images(16, 32, 101) * torch.linspace(0.2, 1.0, 16).view(16, 1, 1, 1)).to(DEV)


def test_apply_attack_and_generate_attack_on_the_vit(tiny):
    from nested_diffusion_amd.attack import apply_attack
    from nested_diffusion_amd.square import SquareL2Attack
    vit, x = tiny, graded_images()[:8].contiguous()
    y = vit.forward(x).argmax(1)
    y[2] = 1 - y[2]
    eps = 2.0
    atk = SquareL2Attack(vit, eps=eps, n_queries=40, seed=3)
    assert atk.model is vit and atk.device == vit.device
    adv = apply_attack(atk, x, y, atk.attack_type, first_image=40)
    adv2, success = atk.generate_attack(x, y, first_image=40)
    assert torch.equal(adv, adv2)                                  # keyed draws: the same call gives the same bits
    pred = vit.forward(adv).argmax(1)
    assert torch.equal(success, pred != y)
    changed = (adv != x).flatten(1).any(1)
    assert not bool(changed[2]) and bool((changed == (success & (torch.arange(8, device=DEV) != 2))).all())
    n = x[0].numel()
    assert float((adv.double() - x.double()).flatten(1).norm(dim=1).max()) <= eps * (1 + (n + 8) * U) + np.sqrt(n) * U
    print(f"square l2 on the tiny ViT: eps {eps}, 40 queries fool {int(changed.sum())} of 7 robust rows")


def test_worst_case_is_the_union_of_apgd_l2_and_square_l2(tiny):
    from nested_diffusion_amd.autoattack import APGDAttack, WorstCase
    from nested_diffusion_amd.square import SquareL2Attack
    vit, x = tiny, graded_images()
    B = x.shape[0]
    y = vit.forward(x).argmax(1)
    y[5] = 1 - y[5]                                                # the clean model gets row 5 wrong
    eps, index = 0.5, 200 + torch.arange(B, device=DEV)
    members = lambda: [APGDAttack(vit, norm="L2", eps=eps, n_iter=10, n_restarts=1, seed=1),      # noqa: E731
                       SquareL2Attack(vit, eps=eps, n_queries=60, seed=1)]
    wc = WorstCase(vit, members())
    adv = wc.perturb(x, y, index=index)
    apgd, square = members()
    robust = torch.arange(B, device=DEV) != 5
    adv_a = apgd.perturb(x[robust].contiguous(), y[robust].contiguous(), index=index[robust])
    fooled_a = torch.zeros(B, dtype=torch.bool, device=DEV)
    fooled_a[robust] = vit.forward(adv_a).argmax(1) != y[robust]
    rest = robust & ~fooled_a
    adv_s = square.perturb(x[rest].contiguous(), y[rest].contiguous(), index=index[rest])
    fooled_s = torch.zeros(B, dtype=torch.bool, device=DEV)
    fooled_s[rest] = vit.forward(adv_s).argmax(1) != y[rest]
    want = x.clone()
    want[fooled_a] = adv_a[fooled_a[robust]]
    want[fooled_s] = adv_s[fooled_s[rest]]
    assert torch.equal(adv, want)
    assert wc.robust_after == [("clean", B - 1), ("APGD", int(rest.sum())), ("SQUAREL2", int((rest & ~fooled_s).sum()))]
    changed = (adv != x).flatten(1).any(1)
    assert torch.equal(changed, fooled_a | fooled_s) and not bool(changed[5])
    adv2, success = wc.generate_attack(x, y, first_image=200)
    assert torch.equal(adv2, adv) and torch.equal(success, vit.forward(adv).argmax(1) != y)
    print(f"worst case at eps {eps}: robust after {wc.robust_after}")


def test_square_l2_on_an_ensemble_target_with_fixed_noise():
    from nested_diffusion_amd.ensemble_grad import EnsembleTarget
    from test_gpu_cond_grad import build_model
    from test_gpu_ensemble_grad import D_IMG, F_DIM, H_DIM, IMG, TAU, config_of, gen
    K, T, B = 2, 4, 3
    cond, _, _ = build_model(2, IMG, (48, 32, 16))
    nets = [ref_cpu.init_cond_model_params(D_IMG, H_DIM, F_DIM, 2, T, seed=60 + k, denoiser=False) for k in range(K)]
    target = EnsembleTarget(cond, nets, config_of(T), mc=2, members=[0, 1], temperature=TAU, seed=4)
    target.fix_noise(B=B)
    x = torch.rand(B, 3, IMG, IMG, generator=gen(31)).to(DEV)
    y = target.forward(x).argmax(1)
    eps, index = 1.0, torch.arange(B, device=DEV)
    runs = []
    for _ in range(2):
        atk = attack(predict=target.forward, eps=eps, n_queries=8, seed=2, check_every=0, device=DEV)
        hist = []
        n_q, x_best = atk.attack_single_run(x, y, index, trace=lambda i, sc, arrays, st: hist.append(st.loss_min.clone()))
        runs.append((n_q.clone(), x_best.clone(), torch.stack(hist)))
    assert all(torch.equal(a, b) for a, b in zip(*runs))           # one pinned sample path: the attack is deterministic
    n_q, x_best, lm = runs[0]
    assert lm.shape == (9, B) and bool((lm[1:] <= lm[:-1]).all()) and bool((n_q >= 1).all()) and bool((n_q <= 9).all())
    assert bool(x_best.isfinite().all()) and float(x_best.min()) >= 0 and float(x_best.max()) <= 1
    assert float((x_best.double() - x.double()).flatten(1).norm(dim=1).max()) <= eps * (1 + (D_IMG + 8) * U) + np.sqrt(D_IMG) * U


def test_write_attacked_set_squarel2(tmp_path):
    import yaml
    from nested_diffusion_amd import main as nd_main
    from nested_diffusion_amd import make_attacks
    from nested_diffusion_amd.data import ImageFolderDataset
    from nested_diffusion_amd.square import SquareL2Attack
    from test_gpu_attack_e2e import _reload_png
    from test_gpu_cli import _write_image_tree, _write_run
    tmp = str(tmp_path)
    ypath, *_ = _write_run(tmp, T=6, K=5, B=3, img=224)
    dataroot = os.path.join(tmp, "data")
    _write_image_tree(dataroot)
    clean = ImageFolderDataset(os.path.join(dataroot, "testing"), "ChestXRay", "grayscaled")
    with open(ypath) as f:
        config = nd_main.dict2namespace(yaml.safe_load(f))
    device = torch.device("cuda", 0)
    out, eps = os.path.join(tmp, "attacked"), 2.0
    atk = SquareL2Attack(make_attacks.load_vit(config, device), eps=eps, n_queries=6, seed=3)
    make_attacks.write_attacked_set(config, atk, "SQUAREL2", out, batch_size=3, dataroot=dataroot)
    tree = os.path.join(out, "Test_attacks_SQUAREL2")
    assert sorted(os.listdir(tree)) == ["NORMAL", "PNEUMONIA"]
    n = 0
    for path, target in clean.samples:
        cls = os.path.basename(os.path.dirname(path))
        stem = os.path.splitext(os.path.basename(path))[0]
        adv = _reload_png(os.path.join(tree, cls, stem + ".png"))
        x, _ = clean[clean.samples.index((path, target))]
        # eps, plus the rounding to 8 bits: at most 0.5 / 255 on each of the 3 * 224 * 224 elements
        assert float((adv.double() - x.double()).norm()) <= eps * (1 + 1e-5) + 0.5 / 255 * np.sqrt(3 * 224 * 224) + 1e-6
        n += 1
    assert n == 7
