"""Edge and scale cases of the L2 and Carlini & Wagner entry points (csrc/nd_attack_l2.hip: nd_l2_step, nd_l2_random_start, nd_cw_attack_space,
nd_cw_model_space, nd_cw_control, nd_cw_update; csrc/nd_vit_grad.hip: nd_margin_head_bwd), each driven alone through nested_diffusion_amd.ops:
the second and third trips of the grid-stride loops past the 256-workgroup cap of a row (and the full workspace that comes with it) and past
the 8192-workgroup cap of the flat pass, the random start's tail quad wherever it lands, the counter's wrap and both key words, bounds whose
a = (lo + hi) / 2 and b = (hi - lo) / 2 differ, the rows of nd_l2_step that take no step, batch tails of the one-thread-per-image kernel,
ragged trips of the margin head, non-finite gradients, the wrappers' refusals, a side stream, and the host arithmetic of the last of ten
binary-search steps.

Every reference is a float64 or numpy float32 restatement: the elementwise passes bit for bit ("one rounded fp32 op in the listing's
order"), the sums within (per_image + 1) * 2^-24 of the float64 sum over the fp32 terms actually formed, the transcendental passes
within max(4 x the error of torch's CPU float32 on the same inputs, 2^-23 * max(1, |lo|, |hi|)) of float64 (the margin of
EXPERIMENTS.md #41)."""
import numpy as np
import pytest
import torch

import test_gpu_cw
from test_gpu_apgd_edges import ref_argmax, same
from test_gpu_cw import adam32, batch, margin64, tiny  # noqa: F401  (tiny, batch: fixtures)
from test_gpu_l2_attack import PHILOX_TOL, delta32, normals64, rows, run_step, start64, step32

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = float("inf")
F32 = np.float32
# 65536 quads: the 256-workgroup cap reached exactly, one trip; 65537: one thread takes a second trip; 131329: two full trips and a ragged third
PAST_CAP = [262144, 262148, 525316]
# 2097152 quads: the 8192-workgroup cap reached exactly; one quad on a second trip; the batch of 64 images of 3 x 224 x 224
FLAT = [8388608, 8388612, 9633792]
BOUNDS = [(-1.0, 1.0), (0.25, 0.75), (-0.3, 1.1)]       # a != b; the last pair is not representable and its fp32 b is not the double's rounding


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def sum_bound(name, got_sq, want_sq, per, where=""):
    """A device sum of squares against the float64 sum over the fp32 terms actually formed: any summation order of non-negative terms, one
    rounding per product and per add (test_gpu_l2_attack's bound and argument)."""
    tol = (per + 1) * 2.0 ** -24
    rel = np.abs(np.asarray(got_sq, dtype=np.float64) - want_sq) / want_sq
    print(f"{where}: {name} relative error {rel.max():.3e} (bound {tol:.3e})")
    assert (rel <= tol).all(), (name, where, rel, tol)


def rule(name, gpu, cpu32, ref64, scale=1.0, where=""):
    """A transcendental pass against float64: max(4 x the error of torch's CPU float32 on the same inputs, 2^-23 * scale)."""
    e_gpu = float((gpu.cpu().double() - ref64).abs().max())
    e_cpu = float((cpu32.double() - ref64).abs().max())
    bound = max(4 * e_cpu, 2.0 ** -23 * scale)
    print(f"{where}: {name} max error against float64: GPU {e_gpu:.3e}, torch CPU float32 {e_cpu:.3e} (bound {bound:.3e})")
    assert e_gpu <= bound, (name, where, e_gpu, bound)


def ab32(lo, hi):
    """a and b as the launches form them: float32 arithmetic on the float32 bounds; as Python floats."""
    lo, hi = F32(lo), F32(hi)
    return float((lo + hi) / F32(2.0)), float((hi - lo) / F32(2.0))


def ab64(lo, hi):
    """a and b as the header defines them, in double from the float32 bounds."""
    lo, hi = float(F32(lo)), float(F32(hi))
    return (lo + hi) / 2.0, (hi - lo) / 2.0


# ---- 1. the row kernels past the 256-workgroup cap -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", PAST_CAP)
def test_l2_step_past_the_workgroup_cap(per):
    B = 3
    x, x0, g = rows(B, per, 1000 + per)
    far = x0 + (x - x0) * F32(40.0)
    #      a step that is projected back, one that stays inside the ball, the final clip_perturbation
    for xx, grad, alpha, eps, lo, hi in ((x, g, 50.0, 0.5, 0.0, 1.0), (x, g, 1e-3, 100.0, 0.0, 1.0), (far, None, 0.0, 0.5, -INF, INF)):
        where = f"per_image={per} alpha={alpha} eps={eps}"
        out, gn, dn = run_step(xx, x0, grad, alpha, eps, lo, hi)
        assert ((dn < eps) if eps > 1 else (dn > eps)).all()
        d = delta32(xx, x0, grad, gn, alpha)                 # the fp32 d actually formed
        want_d = (d.astype(np.float64) ** 2).sum(axis=1)
        sum_bound("dnorm^2", dn.astype(np.float64) ** 2, want_d, per, where)
        if grad is None:
            assert (gn == 0).all()
        else:
            want_g = (grad.astype(np.float64) ** 2).sum(axis=1)
            sum_bound("gnorm^2", gn.astype(np.float64) ** 2, want_g, per, where)
            # the workspace is full at 256 partials per image: the last row of the gradient's partials ends where the first row of d's begins
            sum_bound("gnorm^2 of the last row", gn[B - 1:].astype(np.float64) ** 2, want_g[B - 1:], per, where)
            sum_bound("dnorm^2 of row 0", dn[:1].astype(np.float64) ** 2, want_d[:1], per, where)
        want = step32(xx, x0, grad, gn, dn, alpha, eps, lo, hi)
        same("out", out, want, where)
        same("out, the quad of the last trip", out[:, -4:], want[:, -4:], where)
        out2, gn2, dn2 = run_step(xx, x0, grad, alpha, eps, lo, hi)
        same("out again", out2, out, where), same("gnorm again", gn2, gn, where), same("dnorm again", dn2, dn, where)
        # a row's norms do not depend on the batch around it
        out1, gn1, dn1 = run_step(xx[1:2], x0[1:2], None if grad is None else grad[1:2], alpha, eps, lo, hi)
        same("row 1 alone: gnorm", gn1, gn[1:2], where), same("row 1 alone: dnorm", dn1, dn[1:2], where), same("row 1 alone", out1, out[1:2], where)


def cw_case(B, per, seed, lo=0.0, hi=1.0):
    """x0 inside [lo, hi] with both ends planted, a delta, and the device's w0, xrec and state."""
    from nested_diffusion_amd import ops
    g = torch.Generator().manual_seed(seed)
    lo32, hi32 = float(F32(lo)), float(F32(hi))
    x0 = (lo32 + (hi32 - lo32) * torch.rand(B, per, generator=g)).clamp(lo32, hi32)
    x0[0, :2] = torch.tensor([lo32, hi32])
    x0[B - 1, -2:] = torch.tensor([hi32, lo32])
    delta = 0.3 * torch.randn(B, per, generator=g)
    x0d = x0.to(DEV)
    w0, xrec = ops.cw_attack_space(x0d, lo, hi)
    s = ops.CwState(x0d)
    s.delta.copy_(delta)
    return dict(g=g, x0=x0, x0d=x0d, delta=delta, w0=w0, xrec=xrec, s=s)


def check_model_space(c, per, lo, hi, where):
    """nd_cw_model_space on the case: t and x against float64 (from the device's own w0), the two sums, and a second run."""
    from nested_diffusion_amd import ops
    s, w0, xrec, x0d, delta = c["s"], c["w0"], c["xrec"], c["x0d"], c["delta"]
    a32, b32 = ab32(lo, hi)
    a64, b64 = ab64(lo, hi)
    scale = max(1.0, abs(lo), abs(hi))
    x = ops.cw_model_space(w0, x0d, xrec, s, lo, hi)
    assert x is s.x and torch.isfinite(s.t).all()
    t64 = torch.tanh(w0.cpu().double() + delta.double())
    t32 = torch.tanh(w0.cpu() + delta)
    rule("t", s.t, t32, t64, 1.0, where)
    rule("x", x, t32 * b32 + a32, t64 * b64 + a64, scale, where)
    xn, x0n, rn = x.cpu().numpy(), c["x0"].numpy(), xrec.cpu().numpy()
    for got, diff, name in ((s.sq_rec, xn - rn, "sq_rec"), (s.sq_x0, xn - x0n, "sq_x0")):
        sum_bound(name, got.cpu().double().numpy(), (diff.astype(np.float64) ** 2).sum(axis=1), per, where)
    first = [t.clone() for t in (s.t, s.x, s.sq_rec, s.sq_x0)]
    ops.cw_model_space(w0, x0d, xrec, s, lo, hi)
    for name, a, b in zip(("t", "x", "sq_rec", "sq_x0"), (s.t, s.x, s.sq_rec, s.sq_x0), first):
        same(name + " again", a, b, where)


@pytest.mark.parametrize("per", PAST_CAP)
def test_cw_model_space_past_the_workgroup_cap(per):
    from nested_diffusion_amd import ops
    c = cw_case(3, per, 2000 + per)
    check_model_space(c, per, 0.0, 1.0, f"per_image={per}")
    s = c["s"]
    s.delta.zero_()
    same("x at delta = 0", ops.cw_model_space(c["w0"], c["x0d"], c["xrec"], s), c["xrec"], f"per_image={per}")
    assert not s.sq_rec.any()


def check_update(c, per, steps, lo, hi, where):
    """nd_cw_update on the case, once per (k, flags) of steps: delta, m, v bit for bit against adam32 with the b of the model-space pass; best
    changes exactly in the flagged rows."""
    from nested_diffusion_amd import ops
    s, w0, xrec, x0d = c["s"], c["w0"], c["xrec"], c["x0d"]
    B = s.B
    b_half = (F32(hi) - F32(lo)) / F32(2.0)                  # as nd_cw_model_space's launch forms it
    s.best.fill_(7.0)
    for k, flags in steps:
        x = ops.cw_model_space(w0, x0d, xrec, s, lo, hi).clone()       # the device's own t and x
        dx = (torch.randn(B, per, generator=c["g"]) * 10.0 ** (k % 3 - 1)).to(DEV)
        s.flags.copy_(torch.tensor(flags, dtype=torch.int32))
        before = [a.cpu().numpy().copy() for a in (s.delta, s.m, s.v)]
        best_before = s.best.clone()
        ops.cw_update(s, dx, xrec, 0.01, k, lo, hi)
        want = adam32(*before, dx.cpu().numpy(), x.cpu().numpy(), xrec.cpu().numpy(), s.t.cpu().numpy(), 0.01, k, b_half)
        for got, w, name in zip((s.delta, s.m, s.v), want, ("delta", "m", "v")):
            same(name, got, w, f"{where} k={k}")
        for b in range(B):
            same("best", s.best[b], x[b] if flags[b] else best_before[b], f"{where} k={k} row {b}")
            same("best, the last quad", s.best[b, -4:], x[b, -4:] if flags[b] else best_before[b, -4:], f"{where} k={k} row {b}")
        same("x", s.x, x, f"{where} k={k}")


@pytest.mark.parametrize("per", PAST_CAP)
def test_cw_update_past_the_workgroup_cap(per):
    c = cw_case(3, per, 3000 + per)
    check_update(c, per, ((0, [1, 0, 1]), (999, [1, 0, 1])), 0.0, 1.0, f"per_image={per}")
    assert bool((c["s"].best[1] == 7.0).all()) and not bool((c["s"].best[0] == 7.0).any())


def check_start(x0, eps, seed, first_image=0, restart=0):
    """test_random_start's checks of one nd_l2_random_start call: the point in the unit ball against start64, snorm against normals64, and
    the same bits on a second run.  Returns (out, snorm)."""
    from nested_diffusion_amd import ops
    B, per = x0.shape[0], x0[0].numel()
    where = f"per_image={per} first_image={first_image:#x} restart={restart:#x} seed={seed:#x}"
    out, sn = ops.l2_random_start(x0.to(DEV), eps, seed, first_image, restart, -INF, INF, want_norm=True)
    z = normals64(B, per, seed, first_image, restart)
    total = (z * z).sum(axis=1)
    assert total.min() >= 1.0                               # the tolerance's premise: dividing by ||z|| does not magnify a normal's error
    err = np.abs((out.cpu().double() - x0.double()).numpy() / eps - start64(x0, eps, seed, first_image, restart)).max()
    tol = 2 * PHILOX_TOL + 2.0 ** -23     # the division by ||z|| >= 1 and the norm's own error at most double a normal's; the fp32 add
    print(f"{where}: max |(out - x0) / eps - r| = {err:.3e} (bound {tol:.3e})")
    assert err <= tol, where
    sn_tol = (per + 3) * 2.0 ** -24 + 4 * PHILOX_TOL
    sn_err = np.abs(sn.cpu().double().numpy() ** 2 / total - 1).max()
    print(f"{where}: snorm^2 relative error {sn_err:.3e} (bound {sn_tol:.3e})")
    assert sn_err <= sn_tol, where
    assert float((out.cpu().double() - x0.double()).flatten(1).norm(dim=1).max()) <= eps        # inside the ball before clipping
    again, sn2 = ops.l2_random_start(x0.to(DEV), eps, seed, first_image, restart, -INF, INF, want_norm=True)
    same("start again", again, out, where), same("snorm again", sn2, sn, where)
    return out, sn


@pytest.mark.parametrize("per", PAST_CAP)
def test_random_start_past_the_workgroup_cap(per):
    from nested_diffusion_amd import ops
    x0 = torch.rand(3, per, generator=torch.Generator().manual_seed(4000 + per))
    out, sn = check_start(x0, 1.0, 0x1234_5678_9ABC)
    sub, sn_sub = ops.l2_random_start(x0[1:].to(DEV), 1.0, 0x1234_5678_9ABC, 1, 0, -INF, INF, want_norm=True)
    same("the sub-batch at first_image = 1", sub, out[1:]), same("its snorm", sn_sub, sn[1:])


# ---- 2. nd_cw_attack_space past 8192 workgroups ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", FLAT)
def test_cw_attack_space_past_the_grid_cap(n):
    from nested_diffusion_amd import ops
    cap = FLAT[0]
    x0 = torch.rand(n, generator=torch.Generator().manual_seed(5000))
    plant = torch.tensor([0.0, 1.0, 0.5, 1 - 2.0 ** -24])
    x0[:4] = plant
    x0[-4:] = plant
    if n > cap:
        x0[cap:cap + 4] = plant                             # quad 2097152: the first of the second trip
    w0, xrec = ops.cw_attack_space(x0.to(DEV))
    assert bool(torch.isfinite(w0).all())
    y64 = ((x0.double() - 0.5) / 0.5) * 0.999999
    w64 = torch.atanh(y64)
    w32 = torch.atanh(((x0 - 0.5) / 0.5) * 0.999999)
    rule("w0", w0, w32, w64, where=f"n={n}")
    rule("xrec", xrec, torch.tanh(w32) * 0.5 + 0.5, torch.tanh(w64) * 0.5 + 0.5, where=f"n={n}")
    # an element's result does not depend on n
    wp, rp = ops.cw_attack_space(x0[:cap].to(DEV))
    same("w0 of the prefix", w0[:cap], wp, f"n={n}"), same("xrec of the prefix", xrec[:cap], rp, f"n={n}")
    if n > cap:                                             # and the planted quad of the second trip is the planted first quad
        same("w0 of quad 2097152", w0[cap:cap + 4], w0[:4]), same("xrec of quad 2097152", xrec[cap:cap + 4], xrec[:4])
    same("w0 of the last quad", w0[-4:], w0[:4]), same("xrec of the last quad", xrec[-4:], xrec[:4])


# ---- 3. the random start's tail quad, the counter's wrap, the key words -----------------------------------------------------------------------
# per_image -> a seed, searched on the CPU, at which the tail quad is visible in every image's norm (the condition is asserted below)
TAIL_SEEDS = {4: 0x1234_5678_9ABC, 8: 0x1234_5678_9ABC, 1024: 0x1234_5678_9ABF, 2048: 0x1234_5678_9C03}


@pytest.mark.parametrize("per", [4, 8, 1024, 2048])
def test_random_start_tail_quad(per):
    """The tail quad q == per_image / 4 supplies normals n and n + 1 and discards its other two: thread 1 at per_image 4, thread 2 at 8, and
    thread 0 of workgroup 0 on a second trip where per_image / 4 is a multiple of 256."""
    from nested_diffusion_amd import ops
    B, seed, eps = (2 if per == 2048 else 4), TAIL_SEEDS[per], 1.0
    # only snorm sees the tail: losing normals n and n + 1, or keeping the two discarded ones, must move every image's sum by at least
    # 4 x the tolerance of the check, or the check could not tell
    z = normals64(B, per + 4, seed, 0, 0)                   # one quad further: elements per + 2, per + 3 are the tail quad's discarded normals
    assert np.array_equal(z[:, :per + 2], normals64(B, per, seed, 0, 0))
    total = (z[:, :per + 2] ** 2).sum(axis=1)
    sn_tol = (per + 3) * 2.0 ** -24 + 4 * PHILOX_TOL
    dropped = (z[:, per:per + 2] ** 2).sum(axis=1) / total
    kept = (z[:, per + 2:per + 4] ** 2).sum(axis=1) / total
    print(f"per_image={per}: the tail moves snorm^2 by {dropped.min() / sn_tol:.1f} x (dropped) and {kept.min() / sn_tol:.1f} x (kept) its tolerance")
    assert (dropped >= 4 * sn_tol).all() and (kept >= 4 * sn_tol).all()
    x0 = torch.rand(B, per, generator=torch.Generator().manual_seed(6000 + per))
    out, sn = check_start(x0, eps, seed)
    h = B // 2                                              # keyed on the global image index: a sub-batch draws what it draws in the full batch
    sub, sn_sub = ops.l2_random_start(x0[h:].to(DEV), eps, seed, h, 0, -INF, INF, want_norm=True)
    same("the sub-batch", sub, out[h:]), same("its snorm", sn_sub, sn[h:])
    other, _ = check_start(x0, eps, seed, restart=1)
    assert not torch.equal(other, out)
    same("clipped", ops.l2_random_start(x0.to(DEV), eps, seed, 0, 0), out.clamp(0, 1))


def test_random_start_counter_wrap_and_key_words():
    from nested_diffusion_amd import ops
    B, per, eps = 4, 1028, 1.0
    x0 = torch.rand(B, per, generator=torch.Generator().manual_seed(6100))
    # the image counter wraps: 0xFFFFFFFE, 0xFFFFFFFF, 0, 1
    seed = 0x1234_5678_9ABC
    out, sn = check_start(x0, eps, seed, first_image=0xFFFFFFFE)
    low, sn_low = ops.l2_random_start(x0[2:].to(DEV), eps, seed, 0, 0, -INF, INF, want_norm=True)
    same("images 0 and 1 after the wrap", out[2:], low), same("their snorm", sn[2:], sn_low)
    assert not torch.equal(out[:2] - x0[:2].to(DEV), out[2:] - x0[2:].to(DEV))
    # both key words and the whole restart word count
    seed = 0x8000_0001_0000_0002
    outs = [check_start(x0, eps, s, restart=0xFFFFFFFF)[0] for s in (seed, seed ^ (1 << 40), seed ^ (1 << 3), seed ^ (1 << 63))]
    for i in range(len(outs)):
        for j in range(i):
            assert not torch.equal(outs[i], outs[j]), (i, j)
    assert not torch.equal(check_start(x0, eps, seed, restart=0x7FFFFFFF)[0], outs[0])
    # eps = 0: the clipped image
    x = x0 * 1.5 - 0.25
    same("eps = 0", ops.l2_random_start(x.to(DEV), 0.0, seed, 3, 0xFFFFFFFF, 0.25, 0.75), x.clamp(0.25, 0.75))


# ---- 4. bounds where a != b -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", BOUNDS)
def test_cw_passes_at_bounds_where_a_is_not_b(lo, hi):
    """Measured on the MI355X (EXPERIMENTS.md #43), max absolute error against float64, device / torch CPU float32:
    (-1, 1): w0 6.596e-3 / 6.596e-3, xrec 9.6e-8 / 5.1e-8, t 8.7e-8 / 4.8e-8, x 8.7e-8 / 4.8e-8;
    (0.25, 0.75): w0 6.596e-3 / 6.596e-3, xrec 5.3e-8 / 4.0e-8, t 8.7e-8 / 4.8e-8, x 4.8e-8 / 4.0e-8;
    (-0.3, 1.1): w0 6.596e-3 / 6.596e-3, xrec 1.29e-7 / 9.9e-8, t 8.0e-8 / 5.2e-8, x 1.07e-7 / 1.05e-7.
    w0's error sits at x0 = lo and hi, as at (0, 1): the float32 rounding of 0.999999 * y, which atanh magnifies by 1 / (1 - y^2)."""
    B, per = 3, 768
    where = f"bounds ({lo}, {hi})"
    c = cw_case(B, per, 7000, lo, hi)
    x0 = c["x0"]
    a32, b32 = ab32(lo, hi)
    a64, b64 = ab64(lo, hi)
    scale = max(1.0, abs(lo), abs(hi))
    assert a32 != b32 and float(x0.min()) == float(F32(lo)) and float(x0.max()) == float(F32(hi))
    assert bool(torch.isfinite(c["w0"]).all())
    w64 = torch.atanh(((x0.double() - a64) / b64) * 0.999999)
    w32 = torch.atanh(((x0 - a32) / b32) * 0.999999)
    rule("w0", c["w0"], w32, w64, scale, where)
    rule("xrec", c["xrec"], torch.tanh(w32) * b32 + a32, torch.tanh(w64) * b64 + a64, scale, where)
    check_model_space(c, per, lo, hi, where)
    # nd_cw_update with the b that produced x
    check_update(c, per, ((0, [1, 0, 1]), (5, [0, 1, 0])), lo, hi, where)


@pytest.mark.parametrize("lo,hi", BOUNDS)
def test_cw_model_space_keeps_t_inside_the_unit_interval(lo, hi):
    from nested_diffusion_amd import ops
    B, per = 3, 768
    c = cw_case(B, per, 7100, lo, hi)
    g = c["g"]
    w = torch.empty(B, per)
    w[0] = torch.linspace(-20, 20, per)
    w[1] = 12.0 * torch.randn(per, generator=g)
    w[1, :10] = torch.tensor([88.0, -88.0, INF, -INF, 10.0, -10.0, 10.5, -10.5, 0.0, -0.0])
    w[2] = 5.0 * torch.randn(per, generator=g)
    w[2, -4:] = torch.tensor([-INF, INF, -88.0, 88.0])
    s = c["s"]
    ts = []
    for w0, delta in ((w, torch.zeros(B, per)), (torch.zeros(B, per), w), (w * 0.5, w * 0.5)):
        s.delta.copy_(delta)
        x = ops.cw_model_space(w0.to(DEV), c["x0d"], c["xrec"], s, lo, hi).cpu()
        t = s.t.cpu()
        ts.append(t)
        assert not bool(torch.isnan(t).any()) and float(t.abs().max()) <= 1.0
        big = w.abs() >= 10
        assert int(big.sum()) > per // 2
        same("t where |w| >= 10", t[big], torch.sign(w[big]))
        assert bool(torch.isfinite(x).all())
        if float(F32(lo)) == lo and float(F32(hi)) == hi:    # representable bounds: b + a and -b + a are hi and lo exactly
            assert float(x.min()) == lo and float(x.max()) == hi
        assert bool(torch.isfinite(s.sq_rec).all()) and bool(torch.isfinite(s.sq_x0).all())
    same("t of 0 + w", ts[1], ts[0])


def test_l2_step_at_bounds_minus_one_one():
    B, per = 3, 1028
    rng = np.random.default_rng(7200)
    x0 = (F32(2.0) * rng.random((B, per), dtype=np.float32) - F32(1.0))
    x = np.clip(x0 + F32(0.05) * rng.standard_normal((B, per), dtype=np.float32), F32(-1), F32(1))
    g = rng.standard_normal((B, per), dtype=np.float32)
    out, gn, dn = run_step(x, x0, g, 50.0, 60.0, -1.0, 1.0)
    same("out", out, step32(x, x0, g, gn, dn, 50.0, 60.0, -1.0, 1.0))
    for b in range(B):                                       # the clamp cut every row on both sides
        assert (out[b] == -1).sum() > 10 and (out[b] == 1).sum() > 10 and ((out[b] > -1) & (out[b] < 1)).sum() > 10


# ---- 5. nd_l2_step's special rows -------------------------------------------------------------------------------------------------------------
def special_rows():
    """B = 6, per_image 3072: row 0 a gradient whose squares overflow, 1 one whose squares flush to zero, 2 one +inf element, 3 x == x0 with
    g = 0, 4 x outside [0, 1], 5 ordinary."""
    B, per = 6, 3072
    x, x0, g = rows(B, per, 8000, scale=False)
    q = lambda a: np.round(a * F32(4096)) / F32(4096)        # noqa: E731  on a 2^-12 grid x0 + (x - x0) is x exactly
    x[[0, 2]], x0[[0, 2]] = q(x[[0, 2]]), q(x0[[0, 2]])
    g[0] = 1e20
    g[1] = 1e-25
    g[2, 777] = np.inf
    x[3], g[3] = x0[3], 0.0
    x[4] = x0[4] + F32(0.8) * np.random.default_rng(8001).standard_normal(per, dtype=np.float32)
    assert (x[4] < 0).any() and (x[4] > 1).any()
    return x, x0, g


def test_l2_step_special_rows():
    x, x0, g = special_rows()
    per = x.shape[1]
    alpha, eps = 0.25, 100.0
    out, gn, dn = run_step(x, x0, g, alpha, eps)
    assert gn[0] == INF and gn[2] == INF                    # a gnorm that overflows, and an infinite element: no step
    assert np.isfinite(gn[1]) and gn[1] >= 0                 # the squares flush: whether the sum keeps denormals is not part of the contract
    assert gn[3] == 0 and dn[3] == 0
    assert np.isfinite(out).all() and np.isfinite(dn).all()
    same("out", out, step32(x, x0, g, gn, dn, alpha, eps, 0.0, 1.0))
    same("row 0: no step", out[0], x[0]), same("row 2: no step", out[2], x[2])
    same("row 3: clip(x0)", out[3], np.clip(x0[3], F32(0), F32(1)))
    assert out.min() >= 0 and out.max() <= 1 and (out[4] == 0).any() and (out[4] == 1).any()
    assert not np.array_equal(out[5], x[5])
    ok = [4, 5]
    sum_bound("gnorm^2", gn[ok].astype(np.float64) ** 2, (g[ok].astype(np.float64) ** 2).sum(axis=1), per, "special rows")
    ok = [0, 2, 4, 5]
    d = delta32(x, x0, g, gn, alpha)
    sum_bound("dnorm^2", dn[ok].astype(np.float64) ** 2, (d[ok].astype(np.float64) ** 2).sum(axis=1), per, "special rows")
    # eps = 0: the clipped x0, whatever the row
    out, gn0, dn0 = run_step(x, x0, g, alpha, 0.0, 0.1, 0.9)
    same("gnorm at eps = 0", gn0, gn), same("dnorm at eps = 0", dn0, dn)
    same("eps = 0", out, np.clip(x0, F32(0.1), F32(0.9)))
    same("eps = 0 against the restatement", out, step32(x, x0, g, gn0, dn0, alpha, 0.0, 0.1, 0.9))


# ---- 6. nd_cw_control and the margin head at B and C edges -------------------------------------------------------------------------------------
def control_case(B, C, seed):
    """Random logits with planted rows (every 7th row from 0: a maximum in the last column; from 1: the label C - 1; from 2: a tie between
    columns 0 and C - 1; from 3: all NaN; from 4: a NaN in column 0 only; from 5: the label at the maximum), norms with a NaN and an inf in adversarial rows, and a state."""
    rng = np.random.default_rng(seed)
    logits = rng.standard_normal((B, C)).astype(np.float32)
    labels = rng.integers(0, C, B)
    r = np.arange(B)
    logits[r % 7 == 0, C - 1] = 9.0
    labels[r % 7 == 1] = C - 1
    logits[r % 7 == 2, 0] = logits[r % 7 == 2, C - 1] = 9.0
    logits[r % 7 == 3] = np.nan
    logits[r % 7 == 4, 0] = np.nan
    labels[r % 7 == 5] = ref_argmax(logits[r % 7 == 5])       # rows that hold their label: not adversarial at any C
    labels[np.array([i for i in (63, 126) if i < B], dtype=np.int64)] = 0              # rows at a workgroup's edge: adversarial (maximum in the last column)
    consts = rng.random(B, dtype=np.float32) * F32(10)
    margin = rng.standard_normal(B).astype(np.float32)
    margin[r % 5 == 1], margin[r % 5 == 2] = np.nan, 0.0
    sq_rec = rng.random(B, dtype=np.float32)
    sq_x0 = rng.random(B, dtype=np.float32) * F32(9)
    norm = np.sqrt(sq_x0)
    best_norm = np.where(rng.random(B) < 0.3, F32(INF), norm * rng.choice(np.array([0.5, 1.0, 2.0], dtype=np.float32), B)).astype(np.float32)
    found = rng.integers(0, 2, B).astype(np.int32)
    return dict(logits=logits, labels=labels, consts=consts, margin=margin, sq_rec=sq_rec, sq_x0=sq_x0, best_norm=best_norm, found=found)


def ref_cw_control(c, confidence):
    """nd_cw_control in numpy float32 (test_gpu_cw.test_cw_control's host restatement, vectorised)."""
    B = len(c["labels"])
    l = c["logits"].copy()
    l[np.arange(B), c["labels"]] = l[np.arange(B), c["labels"]] + F32(confidence)
    adv = ref_argmax(l) != c["labels"]
    with np.errstate(invalid="ignore"):
        norm = np.sqrt(c["sq_x0"])
        new_best = adv & (norm < c["best_norm"])
        loss = c["consts"] * np.where(c["margin"] > 0, c["margin"], F32(0)) + c["sq_rec"]
    return dict(adv=adv, found=((c["found"] != 0) | adv).astype(np.int32), flags=new_best.astype(np.int32),
                best_norm=np.where(new_best, norm, c["best_norm"]), loss=loss)


@pytest.mark.parametrize("C", [2, 1024])
@pytest.mark.parametrize("B", [1, 64, 65, 128, 130])       # one 64-thread workgroup with one lane, full, one lane past it, two full, a tail in the third
def test_cw_control_batch_and_class_edges(B, C):
    from nested_diffusion_amd import ops
    confidence = 0.25
    c = control_case(B, C, 9000 + B + C)
    adv = ref_cw_control(c, confidence)["adv"]
    if B >= 64:                                              # a NaN and an infinite norm in rows that are adversarial: neither becomes a best
        i_nan, i_inf = np.flatnonzero(adv)[[3, 4]]
        c["sq_x0"][i_nan], c["sq_x0"][i_inf] = np.nan, np.inf
    want = ref_cw_control(c, confidence)
    s = ops.CwState(torch.zeros(B, 4, device=DEV))
    for name in ("sq_rec", "sq_x0", "best_norm", "found"):
        getattr(s, name).copy_(dev(c[name]))
    s.flags.fill_(-7)                                        # a row the kernel skips would keep these
    s.loss.fill_(float("nan"))
    loss = ops.cw_control(dev(c["logits"]), dev(c["labels"]), dev(c["consts"]), dev(c["margin"]), s, confidence)
    assert loss is s.loss
    where = f"B={B} C={C}"
    for name in ("found", "flags", "best_norm", "loss"):
        same(name, getattr(s, name), want[name], where)
    assert not np.isnan(want["best_norm"]).any() and np.isfinite(want["loss"]).all()
    if B >= 64:
        assert want["flags"][i_nan] == 0 and want["flags"][i_inf] == 0 and want["found"][i_nan] == 1
        assert 0 < want["flags"].sum() < B and 0 < want["adv"].sum() < B and (want["found"] > want["adv"]).any()
        edge = [i for i in (63, 126) if i < B]
        assert want["adv"][edge].all()


@pytest.mark.parametrize("B,C,E", [(70, 2, 257), (3, 1024, 1000), (1, 5, 4)])
def test_margin_head_ragged_trips(B, C, E):
    """E = 257: one element on the second trip of the 256-stride loop; 1000: three full trips and a ragged fourth; 4: most lanes idle."""
    from nested_diffusion_amd import ops
    g = torch.Generator().manual_seed(B * C + E)
    logits = torch.randn(B, C, generator=g)
    labels = torch.randint(0, C, (B,), generator=g)
    labels[::2] = logits[::2].argmax(1)                      # every other row holds its label: margin > 0
    consts = torch.rand(B, generator=g) * 5 + 0.5
    w = torch.randn(C, E, generator=g)
    dfeat, margin, other = ops.margin_head_grad(logits.to(DEV), labels, consts.to(DEV), w.to(DEV), 0.5)
    want_m, want_o = margin64(logits, labels, 0.5)
    assert torch.equal(other.cpu().long(), want_o) and torch.equal(margin.cpu(), want_m)
    on = want_m > 0
    assert bool(on[0]) and (B == 1 or not bool(on.all()))
    want = (consts[:, None].double() * (w.double()[labels] - w.double()[want_o])) * on[:, None]
    err = float((dfeat.cpu().double() - want).abs().max())
    bound = 2.0 ** -22 * float(consts.max() * w.abs().max())
    print(f"B={B} C={C} E={E}: max |dfeat - want| = {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    assert not bool(dfeat.cpu()[~on].any()) and bool(dfeat.cpu()[on].all(dim=1).all())


# ---- 7. nd_cw_update with a non-finite dx -----------------------------------------------------------------------------------------------------
def test_cw_update_with_non_finite_dx():
    from nested_diffusion_amd import ops
    B, per = 3, 1028
    c = cw_case(B, per, 10000)
    s = c["s"]
    x = ops.cw_model_space(c["w0"], c["x0d"], c["xrec"], s).clone()
    dx = torch.randn(B, per, generator=c["g"])
    bad = dx.clone()
    bad[0, 1027], bad[1, 513] = float("nan"), INF
    before = [a.clone() for a in (s.delta, s.m, s.v)]
    got = {}
    for name, d in (("finite", dx), ("bad", bad)):
        for a, b in zip((s.delta, s.m, s.v), before):
            a.copy_(b)
        ops.cw_update(s, d.to(DEV), c["xrec"], 0.01, 0, use_flags=False)
        got[name] = [a.cpu().numpy().copy() for a in (s.delta, s.m, s.v)]
        with np.errstate(invalid="ignore"):
            want = adam32(*[b.cpu().numpy() for b in before], d.numpy(), x.cpu().numpy(), c["xrec"].cpu().numpy(), s.t.cpu().numpy(), 0.01, 0)
        for a, w, n in zip(got[name], want, ("delta", "m", "v")):
            assert np.array_equal(a, w, equal_nan=True), (name, n)
    touched = np.zeros((B, per), bool)
    touched[0, 1027] = touched[1, 513] = True
    for a, f, n in zip(got["bad"], got["finite"], ("delta", "m", "v")):
        same(n + " elsewhere", a[~touched], f[~touched])
        same(n + " of row 2", a[2], f[2])
        assert not np.isfinite(a[touched]).any() and np.isfinite(f).all(), n


# ---- 8. the wrappers' refusals, and a side stream ---------------------------------------------------------------------------------------------
def test_wrappers_refuse_and_write_nothing(tiny, batch):
    from nested_diffusion_amd import _lib, ops
    from nested_diffusion_amd.attack import CarliniWagner
    B, per = 3, 1028
    c = cw_case(B, per, 11000)
    s, w0, xrec, x0d = c["s"], c["w0"], c["xrec"], c["x0d"]
    dx = torch.randn(B, per, generator=c["g"]).to(DEV)
    state = ("delta", "m", "v", "t", "x", "best", "best_norm", "sq_rec", "sq_x0", "found", "flags", "loss")
    s.m.fill_(0.5), s.v.fill_(0.25), s.t.fill_(-3.0), s.x.fill_(-4.0), s.best.fill_(7.0)
    for name in ("sq_rec", "sq_x0", "loss"):
        getattr(s, name).fill_(-1.0)
    snap = {n: getattr(s, n).clone() for n in state}
    strided = lambda t: t.t().contiguous().t()               # noqa: E731  the same shape and values, not contiguous
    assert strided(w0).shape == w0.shape and not strided(w0).is_contiguous()
    odd = torch.rand(B, 1030, device=DEV)
    refusals = [
        (ValueError, lambda: ops.cw_model_space(strided(w0), x0d, xrec, s)),
        (ValueError, lambda: ops.cw_model_space(w0, x0d, strided(xrec), s)),
        (ValueError, lambda: ops.cw_update(s, strided(dx), xrec, 0.01, 0)),
        (_lib.NdError, lambda: ops.cw_update(s, dx.double(), xrec, 0.01, 0)),
        (_lib.NdError, lambda: ops.cw_update(s, dx.cpu(), xrec, 0.01, 0)),
        (_lib.NdError, lambda: ops.cw_model_space(w0.double(), x0d, xrec, s)),
        (_lib.NdError, lambda: ops.cw_model_space(w0.cpu(), x0d, xrec, s)),
        (ValueError, lambda: ops.cw_model_space(w0[:2], x0d[:2], xrec[:2], s)),              # a CwState of another shape
        (ValueError, lambda: ops.cw_update(s, dx[:, :1024].contiguous(), xrec, 0.01, 0)),
        (ValueError, lambda: ops.cw_control(torch.zeros(B + 1, 3, device=DEV), torch.zeros(B + 1), torch.ones(B + 1, device=DEV),
                                            torch.ones(B + 1, device=DEV), s)),
        (_lib.NdError, lambda: ops.cw_attack_space(x0d.double())),
        (_lib.NdError, lambda: ops.cw_attack_space(x0d.cpu())),
        (ValueError, lambda: ops.cw_attack_space(odd)),
        (ValueError, lambda: ops.CwState(odd)),
        (_lib.NdError, lambda: ops.l2_step(x0d.double(), x0d.double(), None, 0.1, 1.0)),
        (_lib.NdError, lambda: ops.l2_step(x0d.cpu(), x0d.cpu(), None, 0.1, 1.0)),
        (_lib.NdError, lambda: ops.l2_step(x0d, x0d, dx.double(), 0.1, 1.0)),
        (ValueError, lambda: ops.l2_step(odd, odd, None, 0.1, 1.0)),
        (_lib.NdError, lambda: ops.l2_random_start(x0d.double(), 1.0, 1)),
        (_lib.NdError, lambda: ops.l2_random_start(x0d.cpu(), 1.0, 1)),
        (ValueError, lambda: ops.l2_random_start(odd, 1.0, 1)),
    ]
    for exc, call in refusals:
        with pytest.raises(exc):
            call()
    for n in state:
        same(n + " after the refusals", getattr(s, n), snap[n])
    # a read-only image that is not contiguous is copied, not refused, and gives the same bits
    same("l2_step on strided images", ops.l2_step(strided(x0d), strided(xrec), strided(dx), 0.1, 1.0), ops.l2_step(x0d, xrec, dx, 0.1, 1.0))
    # labels outside [0, C) in the whole attack
    vit = tiny[0]
    x0, labels = batch
    for bad in (torch.tensor([1, 1, 2, 1]), torch.tensor([-1, 1, 1, 1])):
        with pytest.raises(ValueError):
            CarliniWagner(4.0, vit, binary_search_steps=1, steps=1).generate_attack(x0.to(DEV), bad.to(DEV))


def test_side_stream_gives_the_same_bits():
    from nested_diffusion_amd import ops
    x, x0, g = special_rows()
    xd, x0d, gd = dev(x), dev(x0), dev(g)
    B, per = x.shape
    gen = torch.Generator().manual_seed(12000)
    delta, dx = (0.3 * torch.randn(B, per, generator=gen)).to(DEV), torch.randn(B, per, generator=gen).to(DEV)
    logits, labels = torch.randn(B, 3, generator=gen).to(DEV), torch.tensor([0, 1, 2, 0, 1, 2])
    consts, margin = torch.rand(B, generator=gen).to(DEV), torch.randn(B, generator=gen).to(DEV)

    def run():
        step = ops.l2_step(xd, x0d, gd, 0.25, 100.0, want_norms=True)
        start = ops.l2_random_start(x0d, 1.0, 0x1234_5678_9ABC, 5, 2, want_norm=True)
        w0, xrec = ops.cw_attack_space(x0d)
        s = ops.CwState(x0d)
        s.delta.copy_(delta)
        ops.cw_model_space(w0, x0d, xrec, s)
        ops.cw_control(logits, labels, consts, margin, s)
        ops.cw_update(s, dx, xrec, 0.01, 0)
        return list(step) + list(start) + [w0, xrec] + [getattr(s, n) for n in ("delta", "m", "v", "t", "x", "best", "best_norm", "sq_rec", "sq_x0",
                                                                                  "found", "flags", "loss")]

    want = run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = run()
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    assert len(got) == len(want) == 19 and bool(want[-2].any())          # flags: some row became a best
    for i, (a, b) in enumerate(zip(got, want)):
        same(f"result {i}", a, b, "side stream against the default stream")


# ---- 9. the last of ten binary-search steps ---------------------------------------------------------------------------------------------------
def test_tenth_binary_search_step_takes_the_upper_bound(tiny, batch, monkeypatch):
    """binary_search_steps >= 10: the last step runs at min(upper, 1e10).  The constants the device is given, step by step, are those of
    cw64's host arithmetic rounded to float32."""
    from nested_diffusion_amd.attack import CarliniWagner
    vit, vp64, heads, depth, img = tiny
    x0, labels = batch
    given, given64 = [], []
    orig, orig64 = vit.input_grad_margin, test_gpu_cw.margin_grad64

    def spy(x, lab, c, *args, **kw):
        given.append(c.detach().cpu().clone())
        return orig(x, lab, c, *args, **kw)

    def spy64(vp, x, lab, consts, *args, **kw):
        given64.append(consts.clone())
        return orig64(vp, x, lab, consts, *args, **kw)

    monkeypatch.setattr(vit, "input_grad_margin", spy)
    monkeypatch.setattr(test_gpu_cw, "margin_grad64", spy64)
    atk = CarliniWagner(4.0, vit, binary_search_steps=10, steps=1, abort_early=False)
    f32 = lambda v: torch.full((4,), v, dtype=torch.float64).to(torch.float32)                 # noqa: E731
    for lab, found, seq in ((labels, False, [1e-3 * 10 ** i for i in range(9)] + [1e10]),
                            (1 - labels, True, [1e-3 / 2 ** i for i in range(9)] + [1e-3 / 2 ** 8])):
        given.clear(), given64.clear()
        atk.generate_attack(x0.to(DEV), lab.to(DEV))
        assert bool(torch.isfinite(atk.last_best_norm).all()) == found and bool(torch.isinf(atk.last_best_norm).all()) != found
        _, bn64 = test_gpu_cw.cw64(vp64, heads, depth, x0, lab, 4.0, binary_search_steps=10, steps=1, abort_early=False)
        assert bool(torch.isfinite(bn64).all()) == found
        assert len(given) == len(given64) == len(seq) == 10
        for i in range(10):
            assert given[i].dtype == torch.float32 and given64[i].dtype == torch.float64
            assert torch.equal(given[i], given64[i].to(torch.float32)), (found, i, given[i], given64[i])
            assert torch.equal(given[i], f32(seq[i])), (found, i, given[i], seq[i])
        assert not torch.equal(given[9], given[8] * (0.5 if found else 10.0))                    # not the step the search would take next
