"""Edge cases of the three APGD-CE entry points (nd_apgd_random_start, nd_apgd_control, nd_apgd_update in csrc/nd_attack_linf.hip), each driven
directly with designed inputs and no model: partial workgroups and both passes of the grid-stride loops, the batch tail of the control
kernel, every argmax rule (ties, infinities, NaN logits), loss sequences that isolate each arm of the checkpoint rule, the wrap of
loss_steps' row -1, all eight flag values in one batch with a step of its own per row, and control and update chained over 12 iterations.

The contract is "every operation one rounded fp32 op in the listing's order" (nested_diffusion_amd/autoattack.py), so every comparison
is bit for bit (the int32 view of the floats: NaN payloads and signed zeros count) against the float32 restatements below: ref_control
and ref_update transcribe lines 23-35 of that listing in numpy float32, one op per rounding; tests/test_autoattack_host.py checks them
against the independently written HostAPGD on the CPU.  Each sequence test asserts, from the reference's own trace, that the event it
was designed for occurred."""
import numpy as np
import pytest
import torch

from test_gpu_apgd import host_random_start

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32
NOT_PRED, IMPROVED, RESTORE = 1, 2, 4
EPS = 8 / 255
# one partial wave, one wave short of / exactly / just past one 256-thread workgroup (1024 elements), several workgroups plus a quad
PER_IMAGE = [4, 252, 256, 1020, 1024, 1028, 4096 + 4]
# past the 1024-workgroup cap of a row (1,048,576 elements): a partly filled and a full second pass of the grid-stride loops
GRID_STRIDE = [1_049_604, 2_097_156]
SLACK = 192                      # sentinel elements in front of and behind every state array (>= the largest B here)
F_SENT, I_SENT = 3.0e38, -12345  # the sentinels; the live elements are poisoned with NaN / 0x7FFFFFFF before the initialising call
F_STATE, I_STATE = ("step", "loss_best", "loss_best_last_check"), ("reduced_last_check", "acc", "flags")
IMAGE_ARRAYS = ("x", "x_adv", "x_adv_old", "grad", "x_best", "grad_best", "x_best_adv")


# ---- float32 restatements (numpy, CPU) ---------------------------------------------------------------------------------------------------
def ref_argmax(logits):
    """The first maximal index; a NaN never wins in any column; a row of NaNs alone yields 0."""
    l = np.asarray(logits, dtype=f32)
    ok = ~np.isnan(l)
    top = np.where(ok, l, f32(-np.inf)).max(axis=1, keepdims=True)
    hit = ok & (l == top)
    return np.where(hit.any(axis=1), hit.argmax(axis=1), 0).astype(np.int64)


def ref_new_state(B, n_iter):
    s = {n: np.full(B, np.nan, f32) for n in F_STATE}
    s.update({n: np.full(B, 0x7FFFFFFF, np.int32) for n in I_STATE})
    s["loss_steps"] = np.full((n_iter, B), np.nan, f32)
    return s


def ref_control(s, logits, labels, loss, it, k=0, rho=0.75, step0=0.0):
    """nd_apgd_control on the state dict s (in place).  it = -1: lines 19-21 of the listing; else lines 27-28 and, with k > 0, 31-34
    (the image copies of those lines are ref_update's).  Returns what a checkpoint decided, per row, for the tests' event checks."""
    loss = np.asarray(loss, dtype=f32)
    B, n_iter = loss.shape[0], s["loss_steps"].shape[0]
    pred = ref_argmax(logits) == np.asarray(labels, dtype=np.int64)
    if it < 0:
        s["acc"] = pred.astype(np.int32)
        s["loss_best"], s["loss_best_last_check"] = loss.copy(), loss.copy()
        s["reduced_last_check"] = np.ones(B, np.int32)
        s["step"] = np.full(B, f32(step0), f32)
        s["loss_steps"] = np.zeros((n_iter, B), f32)
        s["flags"] = np.zeros(B, np.int32)
        return None
    ev = None
    with np.errstate(invalid="ignore"):
        s["acc"] = ((s["acc"] != 0) & pred).astype(np.int32)
        s["loss_steps"][it] = loss
        imp = loss > s["loss_best"]
        s["loss_best"] = np.where(imp, loss, s["loss_best"])
        osc = np.zeros(B, bool)
        if k > 0:
            cnt = np.zeros(B, f32)
            for c in range(k):
                cnt = cnt + (s["loss_steps"][it - c] > s["loss_steps"][it - c - 1]).astype(f32)      # row -1: the last row, as numpy indexes
            thr = f32(k) * f32(rho)
            count_arm = cnt <= thr
            second_arm = (s["reduced_last_check"] == 0) & (s["loss_best_last_check"] >= s["loss_best"])
            osc = count_arm | second_arm
            ev = dict(cnt=cnt, thr=thr, count_arm=count_arm, second_arm=second_arm, osc=osc, reduced_before=s["reduced_last_check"].copy(),
                      last_check_before=s["loss_best_last_check"].copy(), best=s["loss_best"].copy())
            s["reduced_last_check"] = osc.astype(np.int32)
            s["loss_best_last_check"] = s["loss_best"].copy()
            s["step"] = np.where(osc, s["step"] / f32(2.0), s["step"])
    s["flags"] = (np.where(pred, 0, NOT_PRED) | np.where(imp, IMPROVED, 0) | np.where(osc, RESTORE, 0)).astype(np.int32)
    return ev


def ref_update(a, flags, step, eps, coef, do_step):
    """nd_apgd_update on the dict a of [B, per] float32 arrays (IMAGE_ARRAYS; entries are replaced, never written through).  The flags'
    copies of lines 27, 28 and 34 of the listing, then with do_step lines 23-25 with a = coef; x and grad are read-only."""
    B = a["x_adv"].shape[0]
    f = np.zeros(B, np.int32) if flags is None else np.asarray(flags, dtype=np.int32)
    notp, imp, res = ((f & bit) != 0 for bit in (NOT_PRED, IMPROVED, RESTORE))
    col = lambda m: m.reshape(B, 1)                                 # noqa: E731
    xa, g = a["x_adv"], a["grad"]
    a["x_best_adv"] = np.where(col(notp), xa, a["x_best_adv"])
    a["x_best"] = np.where(col(imp), xa, a["x_best"])
    a["grad_best"] = np.where(col(imp), g, a["grad_best"])
    xa = np.where(col(res), a["x_best"], xa)
    g = np.where(col(res), a["grad_best"], g)
    if not do_step:
        a["x_adv"] = xa
        return
    e, c = f32(eps), f32(coef)
    one_minus_c = f32(1.0) - c
    st = np.asarray(step, dtype=f32).reshape(B, 1)
    with np.errstate(invalid="ignore"):
        lo, hi = a["x"] - e, a["x"] + e
        grad2 = xa - a["x_adv_old"]
        a["x_adv_old"] = xa
        sgn = np.where(g > 0, f32(1.0), np.where(g < 0, f32(-1.0), f32(0.0)))       # sign(NaN) = 0
        z = np.clip(np.minimum(np.maximum(xa + st * sgn, lo), hi), f32(0.0), f32(1.0))
        v = (xa + (z - xa) * c) + grad2 * one_minus_c
        a["x_adv"] = np.clip(np.minimum(np.maximum(v, lo), hi), f32(0.0), f32(1.0))


# ---- helpers --------------------------------------------------------------------------------------------------------------------------
def bits(t):
    t = t.detach().cpu() if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t))
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(name, got, want, where=""):
    """bit for bit; on a mismatch names the first element that differs."""
    g, w = bits(got), bits(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (name, where, g.shape, w.shape, g.dtype, w.dtype)
    if not torch.equal(g, w):
        bad = (g != w).nonzero()
        at = tuple(bad[0].tolist())
        gv = got.detach().cpu()[at] if torch.is_tensor(got) else got[at]
        wv = want.detach().cpu()[at] if torch.is_tensor(want) else want[at]
        raise AssertionError(f"{name} {where}: {bad.shape[0]} of {g.numel()} elements differ, the first at {at}: got {gv!r}, want {wv!r}")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class GuardedState:
    """An ops.ApgdState whose arrays lie inside larger buffers: SLACK sentinel elements in front of and behind each, the live elements
    poisoned.  check() compares the live elements with the reference's and requires every sentinel intact."""

    def __init__(self, B, n_iter):
        from nested_diffusion_amd import ops
        assert B <= SLACK
        self.st = ops.ApgdState(B, n_iter, DEV)
        self.bufs = {}
        for name in F_STATE + I_STATE + ("loss_steps",):
            n = B * n_iter if name == "loss_steps" else B
            is_f = name not in I_STATE
            buf = torch.full((n + 2 * SLACK,), F_SENT if is_f else I_SENT, dtype=torch.float32 if is_f else torch.int32, device=DEV)
            live = buf[SLACK:SLACK + n]
            live.fill_(float("nan") if is_f else 0x7FFFFFFF)
            setattr(self.st, name, live.view(n_iter, B) if name == "loss_steps" else live)
            self.bufs[name] = buf

    def check(self, ref, where):
        for name, buf in self.bufs.items():
            same(name, getattr(self.st, name), ref[name], where)
            host = buf.cpu()
            guard = torch.cat([host[:SLACK], host[-SLACK:]])
            assert bool((guard == (I_SENT if name in I_STATE else F_SENT)).all()), f"{name} {where}: written outside its {ref[name].size} elements"


def drive_control(B, C, n_iter, ks, rho, logits_at, labels, losses, step0=2 * EPS):
    """A whole synthetic run of nd_apgd_control, no update kernel: it = -1, then 0..n_iter-1 with k = ks.get(it, 0); after every call the
    whole state bit for bit against ref_control.  logits_at(it) -> [B, C]; losses [n_iter + 1, B], row 0 the start point's.  Returns
    the reference's trace [(it, k, checkpoint events or None, flags)] and its final state."""
    from nested_diffusion_amd import ops
    gs, ref = GuardedState(B, n_iter), ref_new_state(B, n_iter)
    labels_d = dev(np.asarray(labels, dtype=np.int64))
    trace = []
    for it in range(-1, n_iter):
        k = 0 if it < 0 else ks.get(it, 0)
        logits, loss = np.asarray(logits_at(it), dtype=f32), np.asarray(losses[it + 1], dtype=f32)
        assert logits.shape == (B, C) and loss.shape == (B,)
        flags = ops.apgd_control(dev(logits), labels_d, dev(loss), gs.st, it, k, rho, step0=step0 if it < 0 else 0.0)
        ev = ref_control(ref, logits, labels, loss, it, k, rho, step0=step0 if it < 0 else 0.0)
        assert flags is gs.st.flags
        gs.check(ref, f"after it={it} (k={k}, B={B}, C={C}, rho={rho})")
        trace.append((it, k, ev, ref["flags"].copy()))
    return trace, ref


def random_logits(B, C, seed):
    rng = np.random.default_rng(seed)
    return lambda it: rng.standard_normal((B, C)).astype(f32)


def flag_values(trace):
    return set(int(v) for _, _, _, f in trace for v in f)


# ---- 1. random start -----------------------------------------------------------------------------------------------------------------------
def start_case(B, per, seed, index=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, per, generator=g)
    index = torch.arange(B) * 7 + 3 if index is None else index
    return x, index


@pytest.mark.parametrize("per", PER_IMAGE)
def test_random_start_partial_workgroups(per):
    from nested_diffusion_amd import ops
    x, idx = start_case(3, per, 300 + per, torch.tensor([41, 7, 1000003]))
    got = ops.apgd_random_start(x.to(DEV), idx.to(DEV), EPS, 0xFEED_0000_0000_0011, restart=1)
    same("start", got, host_random_start(x, idx.numpy(), EPS, 0xFEED_0000_0000_0011, 1), f"per_image={per}")


@pytest.mark.parametrize("per", GRID_STRIDE)
def test_random_start_grid_stride(per):
    from nested_diffusion_amd import ops
    x, idx = start_case(2, per, 310, torch.tensor([5, 2]))
    got = ops.apgd_random_start(x.to(DEV), idx.to(DEV), EPS, 77, restart=0)
    want = host_random_start(x, idx.numpy(), EPS, 77, 0)
    same("start", got, want, f"per_image={per}")
    # the normalisation took the whole row's maximum: the draw reaches the box's face somewhere, in either pass
    assert float((want - x).abs().flatten(1).max(1).values.min()) >= EPS * 0.999


def test_random_start_largest_grid_y_and_shared_indices():
    from nested_diffusion_amd import ops
    B, distinct = 65535, 1000
    g = torch.Generator().manual_seed(320)
    perm = torch.randperm(1 << 20, generator=g)[:distinct]
    pick = torch.arange(B) % distinct
    idx = perm[pick]
    x = torch.rand(distinct, 4, generator=g)[pick]                  # rows that share an index share their image
    got = ops.apgd_random_start(x.to(DEV), idx.to(DEV), EPS, 12345, restart=4)
    same("start", got, host_random_start(x, idx.numpy(), EPS, 12345, 4), "B=65535")
    same("shared index", got[distinct:2 * distinct], got[:distinct])
    same("shared index, last rows", got[65 * distinct:], got[:B - 65 * distinct])


@pytest.mark.parametrize("per", [4, 1028])
def test_random_start_zeroes_its_workspace_in_stream(per):
    from nested_diffusion_amd import _lib
    x, idx = start_case(3, per, 330)
    seed = 0x0BAD_CAFE_0000_0001
    x_d, idx_d = x.to(DEV), idx.to(DEV)
    out = torch.full_like(x_d, float("nan"))
    m_ws = torch.full((3,), -1, dtype=torch.int32, device=DEV)    # 0xFFFFFFFF: above the bits of any |t|
    _lib.check(_lib.load().nd_apgd_random_start(x_d.data_ptr(), idx_d.data_ptr(), out.data_ptr(), m_ws.data_ptr(), 3, per, seed, 2, EPS, 0.0, 1.0,
                                                torch.cuda.current_stream().cuda_stream), "nd_apgd_random_start")
    same("start", out, host_random_start(x, idx.numpy(), EPS, seed, 2), f"poisoned workspace, per_image={per}")
    m = m_ws.cpu().view(torch.float32)                              # what is left there: max |t| of each row, in (0, 1]
    assert bool(((m > 0) & (m <= 1)).all())


def test_random_start_bounds_eps_and_index_words():
    from nested_diffusion_amd import ops
    per = 1028
    g = torch.Generator().manual_seed(340)
    x = torch.rand(4, per, generator=g) * 1.5 - 0.75                # inside and outside [-0.5, 0.25]
    x[:, :6] = torch.tensor([-0.5, 0.25, -0.5000001, 0.2500001, -3.0, 3.0])
    idx = torch.tensor([-1, 2 ** 32 + 5, 5, -(2 ** 33) + 9])
    got = ops.apgd_random_start(x.to(DEV), idx.to(DEV), 0.0, 3, restart=0, lo=-0.5, hi=0.25)
    same("eps = 0", got, torch.clamp(x, -0.5, 0.25))
    # only the low word of the index counts: the two's complement of a negative one, and 2^32 + 5 draws what 5 draws
    y = torch.rand(1, per, generator=g).expand(4, per).contiguous()
    got = ops.apgd_random_start(y.to(DEV), idx.to(DEV), EPS, 3, restart=0)
    same("index words", got, host_random_start(y, idx.numpy(), EPS, 3, 0))
    same("2^32 + 5 is 5", got[1], got[2])
    low = ops.apgd_random_start(y.to(DEV), torch.tensor([2 ** 32 - 1, 5, 5, 9]).to(DEV), EPS, 3, restart=0)
    same("the low words", got, low)
    # bounds other than [0, 1] with a draw: images in [0.1, 0.9] stay inside [0, 1] unclipped, so the narrower clip applies to the same sum
    z = torch.rand(4, per, generator=g) * 0.8 + 0.1
    got = ops.apgd_random_start(z.to(DEV), idx.to(DEV), EPS, 3, restart=1, lo=0.25, hi=0.75)
    unclipped = host_random_start(z, idx.numpy(), EPS, 3, 1)
    assert float(unclipped.min()) > 0 and float(unclipped.max()) < 1
    same("lo = 0.25, hi = 0.75", got, torch.clamp(unclipped, 0.25, 0.75))
    assert bool((got.cpu() == 0.25).any()) and bool((got.cpu() == 0.75).any())


# ---- 2. control: batch tails, argmax rules --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_control_batch_tail_and_poisoned_state(B):
    """One 64-thread workgroup short of, exactly, and just past full; the state starts as NaN / 0x7FFFFFFF inside sentinel slack."""
    n_iter, ks = 6, {1: 2, 3: 2, 5: 3}
    rng = np.random.default_rng(400 + B)
    losses = rng.integers(0, 4, (n_iter + 1, B)).astype(f32)        # small integers: ties, so every branch of the rule occurs
    labels = rng.integers(0, 3, B)
    trace, ref = drive_control(B, 3, n_iter, ks, 0.75, random_logits(B, 3, 401 + B), labels, losses)
    if B >= 63:
        assert flag_values(trace) == set(range(8))                  # every flag value occurred in this batch
        assert len(set(ref["step"].tolist())) >= 2                  # and rows halved their step different numbers of times


def designed_logit_rows(C, rng):
    """[(name, row)]: where the maximum lies, ties, infinities and NaNs, at the first, a middle and the last column."""
    rows = []
    base = lambda: rng.standard_normal(C).astype(f32)               # noqa: E731
    for where, at in (("first", 0), ("middle", C // 2), ("last", C - 1)):
        for what, v in (("max", 9.0), ("posinf", np.inf), ("neginf", -np.inf), ("nan", np.nan)):
            r = base()
            r[at] = v
            rows.append((f"{what}_{where}", r))
        for what, fill in (("rest_neginf", -np.inf), ("rest_nan", np.nan)):
            r = np.full(C, fill, f32)
            r[at] = -3.0
            rows.append((f"{what}_{where}", r))
    for name, cols in (("tie_middle_last", (C // 2, C - 1)), ("tie_first_last", (0, C - 1)), ("tie_first_middle", (0, C // 2))):
        r = base()
        r[list(cols)] = 9.0
        rows.append((name, r))
    r = base()
    r[[0, C - 1]] = np.inf
    rows.append(("tie_posinf", r))
    for name, fill in (("all_equal", 1.5), ("all_neginf", -np.inf), ("all_posinf", np.inf), ("all_nan", np.nan)):
        rows.append((name, np.full(C, fill, f32)))
    r = np.full(C, -np.inf, f32)
    r[0] = np.nan
    rows.append(("nan_first_rest_neginf", r))                       # -inf is a number: it beats the NaN
    r = np.full(C, 2.0, f32)
    r[0] = np.nan
    rows.append(("nan_first_rest_tied", r))
    r = base()
    r[0], r[C - 1] = np.nan, np.inf
    rows.append(("nan_first_posinf_last", r))
    return rows


@pytest.mark.parametrize("C", [1, 2, 3, 1000, 1024])
def test_control_argmax_rules(C):
    rng = np.random.default_rng(420 + C)
    rows = designed_logit_rows(C, rng)
    arg = ref_argmax(np.stack([r for _, r in rows]))
    by_name = {n: int(a) for (n, _), a in zip(rows, arg)}
    # the reference follows the stated rule on the designed rows
    assert by_name["all_nan"] == 0 and by_name["all_equal"] == 0 and by_name["all_neginf"] == 0 and by_name["tie_posinf"] == 0
    assert by_name["nan_first"] != 0 or C == 1
    assert by_name["nan_first_rest_neginf"] == min(1, C - 1) and by_name["nan_first_rest_tied"] == min(1, C - 1)
    assert by_name["nan_first_posinf_last"] == C - 1 and by_name["rest_nan_last"] == C - 1 and by_name["rest_nan_middle"] == C // 2
    assert by_name["tie_middle_last"] == C // 2 and by_name["posinf_last"] == C - 1 and by_name["max_last"] == C - 1
    # every row under five labels: the argmax, another class, and three out of range (one whose low word is the argmax)
    logits = np.repeat(np.stack([r for _, r in rows]), 5, axis=0)
    a5 = np.repeat(arg, 5)
    labels = np.stack([arg, (arg + 1) % C if C > 1 else arg + 1, np.full_like(arg, C), np.full_like(arg, -1), arg + 2 ** 32], axis=1).reshape(-1)
    B, n_iter = logits.shape[0], 3
    assert B <= SLACK
    losses = rng.integers(0, 3, (n_iter + 1, B)).astype(f32)
    rolled = {-1: 0, 0: 5, 1: 0, 2: 10}                             # the rows move under the labels: acc &= pred sees both outcomes

    def logits_at(it):
        return np.roll(logits, rolled[it], axis=0)

    trace, ref = drive_control(B, C, n_iter, {2: 3}, 0.75, logits_at, labels, losses)
    pred0 = (a5 == labels).reshape(-1, 5)
    assert bool(pred0[:, 0].all()) and not bool(pred0[:, 2:].any())
    first = {f[0]: f[3] for f in trace}[1]                          # iteration 1 sees the rows unrolled again
    assert bool(((first & NOT_PRED) == 0).reshape(-1, 5)[:, 0].all()) and bool(((first & NOT_PRED) != 0).reshape(-1, 5)[:, 2:].all())
    if C > 1:
        assert 0 < int(ref["acc"].sum()) < B


# ---- 3. control: the checkpoint rule -------------------------------------------------------------------------------------------------------
SEQ_N_ITER, SEQ_K = 132, 4                                          # a checkpoint of length 4 every 4 iterations: 33 of them


def loss_rows(n_iter, k, rng):
    """{name: [n_iter + 1] float32}: element 0 the start point's loss, element i + 1 iteration i's.  Window w is iterations wk..wk+k-1."""
    n_win = n_iter // k
    up = np.arange(k, dtype=f32)
    rows = {}
    rows["rising"] = 1.0 + np.arange(n_iter + 1, dtype=f32)        # k rises in every window: never oscillates by count
    rows["constant"] = np.ones(n_iter + 1, f32)                     # no rise: a restore at every checkpoint
    # a drop at the start of each window, then k - 1 rises: cnt == k - 1 in every window but the first
    rows["drop_then_rises"] = np.concatenate([[1.0]] + [1000.0 - 10.0 * w + up for w in range(n_win)])
    # windows of k - 1 and of k rises in turn
    seq, last = [[1.0]], 100.0
    for w in range(n_win):
        start = last - 5.0 if w % 2 == 0 else last + 1.0
        seq.append(start + up)
        last = start + k - 1
    rows["rises_alternate"] = np.concatenate(seq)
    # a best set in the first window, then windows of k - 1 rises that stay below it: loss_best_last_check == loss_best
    rows["below_the_best"] = np.concatenate([[5.0], 10.0 + up] + [1.0 + up for _ in range(1, n_win)])
    # the same, but each window's last loss is a new best: loss_best_last_check < loss_best
    rows["new_best_each_window"] = np.concatenate([[5.0], 10.0 + up] + [np.concatenate([1.0 + up[:-1], [13.0 + w]]) for w in range(1, n_win)])
    rows["nan_start"] = rows["rising"].copy()
    rows["nan_start"][0] = np.nan                                   # loss_best stays NaN: nothing improves on it
    rows["nan_inside"] = rows["rising"].copy()
    rows["nan_inside"][5::5] = np.nan
    r = rng.integers(0, 4, n_iter + 1).astype(f32)
    r[0], r[10], r[15], r[21], r[40], r[41] = -np.inf, np.inf, -np.inf, np.nan, np.inf, np.inf
    rows["inf_inside"] = r
    rows["all_neginf"] = np.full(n_iter + 1, -np.inf, f32)
    rows["posinf_start"] = np.concatenate([[np.inf], rng.integers(0, 4, n_iter).astype(f32)])
    for j in range(8):
        rows[f"random_int_{j}"] = rng.integers(0, 4, n_iter + 1).astype(f32)
    for j in range(4):
        rows[f"random_{j}"] = rng.standard_normal(n_iter + 1).astype(f32)
    rows = {n: np.asarray(v, dtype=f32) for n, v in rows.items()}  # every designed value is a small integer: exact
    assert all(v.shape == (n_iter + 1,) for v in rows.values())
    return rows


def checkpoints_of(trace, row):
    """the reference's checkpoint events of one row: [dict of scalars]"""
    return [{n: (v[row] if isinstance(v, np.ndarray) else v) for n, v in ev.items()} for _, _, ev, _ in trace if ev is not None]


@pytest.mark.parametrize("rho", [0.75, 0.5])
def test_control_checkpoint_rule_on_designed_loss_sequences(rho):
    n_iter, k = SEQ_N_ITER, SEQ_K
    rows = loss_rows(n_iter, k, np.random.default_rng(500))
    names = list(rows)
    B = len(names)
    losses = np.stack([rows[n] for n in names], axis=1)
    ks = {i: k for i in range(k - 1, n_iter, k)}                    # the first has k = it + 1: its last comparison reads row -1
    labels = np.random.default_rng(501).integers(0, 2, B)
    trace, ref = drive_control(B, 2, n_iter, ks, rho, random_logits(B, 2, 502), labels, losses)
    cp = {n: checkpoints_of(trace, i) for i, n in enumerate(names)}
    n_cp = n_iter // k
    assert all(len(v) == n_cp for v in cp.values()) and n_cp >= 31
    thr = k * rho                                                   # dyadic rho: exact in fp32 and in double
    assert all(float(e["thr"]) == thr for e in cp["rising"])
    # what each sequence was designed for, read off the reference's trace
    assert all(e["cnt"] == k and not e["count_arm"] for e in cp["rising"])
    assert all(e["cnt"] <= 1 and e["count_arm"] and e["osc"] for e in cp["constant"])
    step = ref["step"][names.index("constant")]
    assert step == f32(2 * EPS) / f32(2.0 ** n_cp) and step > 0     # halved at every checkpoint, 33 times, and still a normal number
    assert all(e["cnt"] == k - 1 for e in cp["drop_then_rises"][1:])
    assert {int(e["cnt"]) for e in cp["rises_alternate"]} == {k - 1, k}
    assert all(not e["osc"] for e in cp["nan_start"]) and np.isnan(ref["loss_best"][names.index("nan_start")])
    assert ref["loss_best"][names.index("inf_inside")] == np.inf and np.isneginf(ref["loss_best"][names.index("all_neginf")])
    everything = [e for v in cp.values() for e in v]
    if rho == 0.75:
        # cnt == k * rho exactly: <= fires; its neighbour with one more rise does not fire by count
        assert all(e["cnt"] == thr and e["count_arm"] and e["osc"] for e in cp["drop_then_rises"][1:])
        assert any(e["cnt"] == thr and e["osc"] for e in cp["rises_alternate"])
        assert any(e["cnt"] == thr + 1 and not e["count_arm"] for e in cp["rises_alternate"])
        assert all(not e["osc"] for e in cp["rising"])              # never reduced: the second arm needs an earlier best to hold
    else:
        # the count arm false (k - 1 > k / 2) straight after a checkpoint that did not reduce: the second arm decides alone
        fired = [e for e in cp["below_the_best"] if not e["count_arm"] and e["reduced_before"] == 0]
        assert fired and all(e["last_check_before"] == e["best"] and e["second_arm"] and e["osc"] for e in fired)
        held = [e for e in cp["new_best_each_window"] if not e["count_arm"] and e["reduced_before"] == 0]
        assert len(held) >= 30 and all(e["last_check_before"] < e["best"] and not e["osc"] for e in held)
        assert any(e["cnt"] == thr and e["osc"] for e in everything) and any(e["cnt"] == thr + 1 and not e["count_arm"] for e in everything)
        # and after a checkpoint that did reduce, the second arm is off
        assert any(not e["count_arm"] and e["reduced_before"] == 1 and e["last_check_before"] >= e["best"] and not e["osc"] for e in everything)
    assert flag_values(trace) == set(range(8))                      # control produced every flag value in this run


@pytest.mark.parametrize("rho", [0.75, 0.5])
@pytest.mark.parametrize("n_iter,ks", [(1, {0: 1}), (5, {2: 3, 4: 5}), (4, {0: 1, 1: 2, 3: 4}), (2, {1: 2})])
def test_control_row_minus_one_wraps_to_the_last_row(n_iter, ks, rho):
    """k = it + 1: the last comparison reads row -1, which is row n_iter - 1: row 0 itself at n_iter = 1, still zero before the last
    iteration, and the row just written at it = n_iter - 1."""
    rng = np.random.default_rng(520 + n_iter)
    designed = [[9, 5, 6, 1, 2, 7], [9, 5, 6, 7, 2, 1], [3, 9, 1, 2, 3, 4], [3, 9, 1, 2, 1, 4], [3, 1, 0, 1, 0, 5], [3, 1, 2, 3, 0, 5],
                [np.nan, 1, 2, 3, 4, 5], [2, np.nan, 1, np.inf, -np.inf, np.inf], [0, 0, 0, 0, 0, 0], [1, -1, -2, -3, -4, -5]]
    losses = np.concatenate([np.array(designed, dtype=f32).T[:n_iter + 1], rng.integers(0, 3, (n_iter + 1, 6)).astype(f32)], axis=1)
    B = losses.shape[1]
    trace, ref = drive_control(B, 2, n_iter, ks, rho, random_logits(B, 2, 521), rng.integers(0, 2, B), losses)
    events = [ev for _, _, ev, _ in trace if ev is not None]
    assert len(events) == len(ks)
    if n_iter > 2:                                                  # both outcomes occur (at n_iter <= 2 the two rows cannot both rise)
        assert any(bool(e["osc"].any()) for e in events) and any(not bool(e["osc"].all()) for e in events)
    if n_iter == 1:                                                 # row -1 is row 0: no loss exceeds itself
        assert bool((events[0]["cnt"] == 0).all()) and bool(events[0]["osc"].all())
        assert bool((ref["step"] == f32(2 * EPS) / f32(2.0)).all())
    if n_iter == 5:
        # it = 2 read the last row while it was zero, it = 4 after it was written: both decide a designed row
        # (rows 0-1: 5 > 0 is the deciding rise at it = 2; rows 2-5: loss[0] > loss[4] or not at it = 4)
        assert {bool(events[0]["osc"][0]), bool(events[0]["osc"][1])} == {True, False} or rho == 0.5
        assert len({bool(events[1]["osc"][r]) for r in (2, 3, 4, 5)}) == 2


# ---- 4. update -----------------------------------------------------------------------------------------------------------------------------
STEPS = [2 * EPS, 0.0, 1e-40, EPS, EPS / 4]                         # per row, in turn: 2 eps, none, a denormal, eps, a quarter


def update_case(B, per, seed, eps=EPS):
    """{name: [B, per] float32} of IMAGE_ARRAYS: images at 0, at 1 and within eps of either bound; iterates on the faces of the eps-box;
    gradients with signed zeros, denormals, infinities and NaN; every array its own values; all iterates finite."""
    rng = np.random.default_rng(seed)
    e = f32(eps)
    i = np.arange(B * per, dtype=np.int64).reshape(B, per)
    x = rng.random((B, per), dtype=f32)
    for r, v in ((0, 0.0), (1, 1.0), (2, e * f32(0.5)), (3, f32(1.0) - e * f32(0.5)), (4, e), (5, f32(1.0) - e)):
        x[i % 9 == r] = v
    box = lambda t: np.clip(np.minimum(np.maximum(t, x - e), x + e), f32(0.0), f32(1.0))      # noqa: E731
    inside = lambda: box(x + e * (f32(2.0) * rng.random((B, per), dtype=f32) - f32(1.0)))       # noqa: E731
    a = dict(x=x, x_adv=inside(), x_adv_old=inside(), x_best=inside(), x_best_adv=inside())
    a["x_adv"][i % 5 == 0] = box(x - e)[i % 5 == 0]
    a["x_adv"][i % 5 == 1] = box(x + e)[i % 5 == 1]
    for name, mod in (("grad", 11), ("grad_best", 13)):
        g = rng.standard_normal((B, per)).astype(f32)
        for r, v in enumerate((0.0, -0.0, 1e-40, -1e-40, np.inf, -np.inf, np.nan)):
            g[i % mod == r] = v
        a[name] = g
    assert all(np.isfinite(a[n]).all() for n in ("x", "x_adv", "x_adv_old", "x_best", "x_best_adv"))
    assert bool((a["x_adv"] != a["x_adv_old"]).any())
    return a


def run_update(a, flags, step, coef, do_step, where, eps=EPS):
    """nd_apgd_update on device copies of the case against ref_update on host copies: all seven arrays bit for bit."""
    from nested_diffusion_amd import ops
    d = {n: dev(v) for n, v in a.items()}
    want = {n: v.copy() for n, v in a.items()}
    flags_d = None if flags is None else dev(np.asarray(flags, dtype=np.int32))
    step_d = dev(np.asarray(step, dtype=f32))
    ops.apgd_update(d["x"], d["x_adv"], d["x_adv_old"], d["grad"], d["x_best"], d["grad_best"], d["x_best_adv"], flags_d, step_d, eps, coef, do_step)
    ref_update(want, flags, step, eps, coef, do_step)
    for n in IMAGE_ARRAYS:
        same(n, d[n], want[n], where)
    return want


def row_steps(B):
    return np.array([STEPS[b % len(STEPS)] for b in range(B)], dtype=f32)


@pytest.mark.parametrize("per", PER_IMAGE)
def test_update_every_flag_value_in_one_batch(per):
    """40 rows: flags b % 8 against steps b % 5, so every flag value meets every step; both coefficients, with and without the step."""
    B = 40
    a = update_case(B, per, 600 + per)
    flags, step = np.arange(B) % 8, row_steps(B)
    assert step[2] > 0 and step[2] < np.finfo(f32).tiny             # the denormal survived the conversion
    for do_step in (False, True):
        for coef in (1.0, 0.75):
            want = run_update(a, flags, step, coef, do_step, f"per_image={per} do_step={do_step} a={coef}")
            # arrays the flags do not select come back as they were, whatever the reference says
            for n, bit in (("x_best_adv", NOT_PRED), ("x_best", IMPROVED), ("grad_best", IMPROVED)):
                same(n + " unselected rows", want[n][(flags & bit) == 0], a[n][(flags & bit) == 0])
            same("grad", want["grad"], a["grad"])
            if not do_step:
                same("x_adv_old", want["x_adv_old"], a["x_adv_old"])
                keep = ((flags & RESTORE) == 0) | ((flags & IMPROVED) != 0)
                same("x_adv unrestored rows", want["x_adv"][keep], a["x_adv"][keep])
    want = run_update(a, None, step, 1.0, True, f"per_image={per} flags=None")
    for n in ("x_best", "grad_best", "x_best_adv"):
        same(n, want[n], a[n])
    # the designed values did something: a NaN gradient made no step (z = x_adv, so only the momentum term moved the iterate)
    want = {n: v.copy() for n, v in a.items()}
    ref_update(want, None, step, EPS, 1.0, True)
    nan_g = np.isnan(a["grad"])
    same("no step on a NaN gradient", want["x_adv"][nan_g], a["x_adv"][nan_g])


@pytest.mark.parametrize("per", GRID_STRIDE)
def test_update_grid_stride(per):
    a = update_case(2, per, 610)
    step = np.array([EPS, EPS / 4], dtype=f32)
    run_update(a, [RESTORE, NOT_PRED | IMPROVED], step, 0.75, True, f"per_image={per} step")
    run_update(a, [NOT_PRED | IMPROVED | RESTORE, RESTORE], step, 0.75, False, f"per_image={per} no step")


def test_update_largest_grid_y():
    B = 65535
    a = update_case(B, 4, 620)
    flags, step = np.arange(B) % 8, row_steps(B)
    run_update(a, flags, step, 0.75, True, "B=65535 step")
    run_update(a, flags, step, 0.75, False, "B=65535 no step")
    run_update(a, None, step, 1.0, True, "B=65535 flags=None")


# ---- 5. control and update chained ------------------------------------------------------------------------------------------------------------
def test_control_then_update_chained_for_12_iterations():
    """attack_single_run's loop on synthetic logits, losses and gradients: the flags control writes are the flags update reads."""
    from nested_diffusion_amd import ops
    B, per, C, n_iter, rho = 9, 1028, 3, 12, 0.75
    ks = {2: 3, 5: 3, 7: 2, 11: 4}
    rng = np.random.default_rng(700)
    a = update_case(B, per, 701)
    a["x_adv_old"], a["x_best"], a["x_best_adv"] = a["x_adv"].copy(), a["x_adv"].copy(), a["x_adv"].copy()
    labels = rng.integers(0, C, B)
    draw = lambda: (rng.standard_normal((B, C)).astype(f32), rng.integers(0, 4, B).astype(f32), update_case(B, per, int(rng.integers(1 << 30)))["grad"])  # noqa: E731
    logits, loss, grad = draw()
    a["grad"], a["grad_best"] = grad, grad.copy()
    gs, ref = GuardedState(B, n_iter), ref_new_state(B, n_iter)
    d = {n: dev(v) for n, v in a.items()}
    labels_d = dev(labels.astype(np.int64))

    def compare(where):
        gs.check(ref, where)
        for n in IMAGE_ARRAYS:
            same(n, d[n], a[n], where)

    ops.apgd_control(dev(logits), labels_d, dev(loss), gs.st, -1, 0, rho, step0=2 * EPS)
    ref_control(ref, logits, labels, loss, -1, 0, rho, step0=2 * EPS)
    ops.apgd_update(d["x"], d["x_adv"], d["x_adv_old"], d["grad"], None, None, None, None, gs.st.step, EPS, 1.0, True)
    ref_update(a, None, ref["step"], EPS, 1.0, True)
    compare("after the first step")
    seen, restored = set(), 0
    for i in range(n_iter):
        logits, loss, grad = draw()
        d["grad"], a["grad"] = dev(grad), grad
        flags = ops.apgd_control(dev(logits), labels_d, dev(loss), gs.st, i, ks.get(i, 0), rho)
        ref_control(ref, logits, labels, loss, i, ks.get(i, 0), rho)
        ops.apgd_update(d["x"], d["x_adv"], d["x_adv_old"], d["grad"], d["x_best"], d["grad_best"], d["x_best_adv"], flags, gs.st.step, EPS, 0.75,
                        i + 1 < n_iter)
        ref_update(a, ref["flags"], ref["step"], EPS, 0.75, i + 1 < n_iter)
        compare(f"after iteration {i}")
        seen |= set(int(v) for v in ref["flags"])
        restored += int(((ref["flags"] & RESTORE) != 0).sum())
    assert restored >= 2 and len(set(ref["step"].tolist())) >= 2    # rows restored, and not all the same number of times
    assert {f & RESTORE for f in seen} == {0, RESTORE} and {f & IMPROVED for f in seen} == {0, IMPROVED} and {f & NOT_PRED for f in seen} == {0, NOT_PRED}
