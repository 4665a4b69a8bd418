"""APGD-L2 and the EOT target on the GPU (csrc/nd_apgd_l2.hip: nd_apgd_l2_random_start, nd_apgd_l2_step, nd_eot_add;
autoattack.APGDAttack(norm='L2'), eot.EOTTarget, make_attacks APGDL2 / --eot): the start against a float64 restatement of the Philox /
Box-Muller draws, the step and every iteration's arrays bit for bit against the float32 restatement of tests/test_apgd_l2_host.py fed
the GPU's norms, the norms against float64 sums, generate_attack's row rules, the attack's strength against L2PGD, the EOT mean bit for
bit, and the attacked tree end to end."""
import os

import numpy as np
import pytest
import torch

from oracle import ref_cpu
from test_apgd_l2_host import APGD_L2_START_TAG, APGD_RESTORE, F32, l2_step32
from test_gpu_apgd import HostAPGD
from test_gpu_attack import images
from test_gpu_l2_attack import PHILOX_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = float("inf")
U = 2.0 ** -24


@pytest.fixture(scope="module")
def tiny():
    from nested_diffusion_amd.mapping import VisionTransformer
    return VisionTransformer(ref_cpu.init_vit_params(embed=128, depth=5, patch=16, img=32, seed=3), 2, DEV)


# ---- 1. the start ---------------------------------------------------------------------------------------------------------------------------
def normals64(index, per, seed, restart):
    """[B, per] float64: the normals nd_apgd_l2_random_start draws (Philox4x32-10 words through the Box-Muller of nd_philox.hpp, the word
    mapping of nd_l2_random_start: words 0, 1 -> normals 0, 1; words 2, 3 -> normals 2, 3)."""
    B, Q = len(index), per // 4
    b, q = np.meshgrid(np.asarray(index, dtype=np.int64), np.arange(Q), indexing="ij")
    ctr = np.stack([b & 0xFFFFFFFF, q, np.full_like(q, restart), np.full_like(q, APGD_L2_START_TAG)], axis=-1).reshape(-1, 4)
    x = ref_cpu.philox4x32_10(ctr, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF).astype(np.float64)
    two32 = 4294967296.0
    u1 = np.minimum(x[:, [0, 2]].astype(np.float32).astype(np.float64) + 1.0, two32) / two32
    u2 = x[:, [1, 3]].astype(np.float32).astype(np.float64) / two32
    r = np.sqrt(-2.0 * np.log(u1))
    z = np.stack([r[:, 0] * np.cos(2 * np.pi * u2[:, 0]), r[:, 0] * np.sin(2 * np.pi * u2[:, 0]),
                  r[:, 1] * np.cos(2 * np.pi * u2[:, 1]), r[:, 1] * np.sin(2 * np.pi * u2[:, 1])], axis=1)
    return z.reshape(B, per)


def check_start(x0, idx, eps, seed, restart):
    """The unclipped start against float64, tnorm against the float64 sum, and the clipped start's box and ball; returns the clipped start."""
    from nested_diffusion_amd import ops
    B, per = x0.shape[0], x0[0].numel()
    raw, tn = ops.apgd_l2_random_start(x0.to(DEV), idx.to(DEV), eps, seed, restart, -INF, INF, want_norm=True)
    t = normals64(idx.numpy(), per, seed, restart)
    sq = (t * t).sum(axis=1)
    want = t / (np.sqrt(sq) + 1e-12).reshape(B, 1)
    got = (raw.cpu().double() - x0.double()).numpy().reshape(B, per) / eps
    err, tol = np.abs(got - want).max(), 2 * PHILOX_TOL + 2.0 ** -23
    rel = np.abs(tn.cpu().double().numpy() ** 2 / sq - 1).max()
    print(f"apgd l2 start per={per}: max |(out - x0) / eps - t / ||t||| = {err:.3e} (bound {tol:.3e}); tnorm^2 relative {rel:.3e} "
          f"(bound {(per + 1) * U:.3e})")
    assert err <= tol
    assert rel <= (per + 1) * U
    s = ops.apgd_l2_random_start(x0.to(DEV), idx.to(DEV), eps, seed, restart)
    assert torch.equal(s, raw.clamp(0, 1))
    assert float(s.min()) >= 0 and float(s.max()) <= 1
    assert float((s.cpu().double() - x0.double()).flatten(1).norm(dim=1).max()) <= eps * (1 + per * U)
    return s


def test_start_against_float64_and_keyed_on_the_global_index():
    from nested_diffusion_amd import ops
    x0 = images(4, 32, 61)
    eps, seed = 0.75, 0x0123_4567_89AB_CDEF
    idx = torch.tensor([10, 11, 12, 13])
    s = check_start(x0, idx, eps, seed, 2)
    sub = ops.apgd_l2_random_start(x0[[1, 3]].to(DEV), idx[[1, 3]].to(DEV), eps, seed, restart=2)   # a compacted restart subset
    assert torch.equal(sub, s[[1, 3]])
    assert torch.equal(ops.apgd_l2_random_start(x0.to(DEV), idx.to(DEV), eps, seed, restart=2), s)
    assert not torch.equal(ops.apgd_l2_random_start(x0.to(DEV), idx.to(DEV), eps, seed, restart=3), s)
    # foolbox's ball at the same key draws with another tag (and n + 2 normals): an independent start
    assert not torch.equal(ops.l2_random_start(x0.to(DEV), eps, seed, 10, 2), s)


def test_start_at_the_production_shape():
    x0 = images(3, 224, 62)
    check_start(x0, torch.tensor([7, 0, 2 ** 32 + 5]), 2.0, 9, 0)            # the counter takes the index's low word
    from nested_diffusion_amd import ops
    a = ops.apgd_l2_random_start(x0[2:].to(DEV), torch.tensor([2 ** 32 + 5]).to(DEV), 2.0, 9, 0)
    assert torch.equal(a, ops.apgd_l2_random_start(x0[2:].to(DEV), torch.tensor([5]).to(DEV), 2.0, 9, 0))


# ---- 2. the step, bit for bit given the norms ----------------------------------------------------------------------------------------------
def step_rows(B, per, seed):
    """x, the iterate xa, the previous iterate xold, and two gradients whose rows differ in magnitude by decades."""
    rng = np.random.default_rng(seed)
    x = rng.random((B, per), dtype=F32)
    xa = np.clip(x + F32(0.05) * rng.standard_normal((B, per), dtype=F32), F32(0), F32(1))
    xold = np.clip(xa + F32(0.02) * rng.standard_normal((B, per), dtype=F32), F32(0), F32(1))
    scale = (F32(10.0) ** np.arange(-2, B - 2, dtype=F32)).reshape(B, 1)
    g = rng.standard_normal((B, per), dtype=F32) * scale
    gb = rng.standard_normal((B, per), dtype=F32) * scale
    return x, xa, xold, g, gb


def run_step(x, xa, xold, g, gb, flags, s, eps, a):
    """(x_adv, x_adv_old, norms) of nd_apgd_l2_step on copies of the arrays."""
    from nested_diffusion_amd import ops
    t = lambda v: torch.from_numpy(v.copy()).to(DEV)          # noqa: E731
    x_adv, x_old = t(xa), t(xold)
    norms = ops.apgd_l2_step(t(x), x_adv, x_old, t(g), None if flags is None else t(gb),
                             None if flags is None else torch.tensor(flags, dtype=torch.int32, device=DEV), t(s), eps, a)
    return x_adv.cpu().numpy(), x_old.cpu().numpy(), norms.cpu().numpy()


def check_step(x, xa, xold, g, gb, flags, s, eps, a):
    """One GPU step against the restatement fed the GPU's norms; the norms against float64; a second run; returns (out, norms)."""
    B, per = x.shape
    out, old, norms = run_step(x, xa, xold, g, gb, flags, s, eps, a)
    used = g.copy()
    if flags is not None:
        restore = (np.asarray(flags) & APGD_RESTORE) != 0
        used[restore] = gb[restore]
    want, want_old, _, (d1, d2) = l2_step32(x, xa, xold, used, s, eps, a, norms=norms)
    assert np.array_equal(old, want_old) and np.array_equal(old, xa)
    assert np.array_equal(out, want, equal_nan=True), float(np.abs(out - want).max())
    tol = (per + 1) * U          # any summation order of non-negative terms, one rounding per product and per add; the root's two
    for k, (name, v) in enumerate((("gn", used), ("n1", d1), ("n2", d2))):
        sq = (v.astype(np.float64) ** 2).sum(axis=1)
        ok = np.isfinite(sq) & (sq > 0)
        rel = np.abs(norms[k].astype(np.float64)[ok] ** 2 - sq[ok]) / sq[ok]
        assert (rel <= tol).all(), (name, rel, tol)
        assert (norms[k][sq == 0] == 0).all()
    out2, old2, norms2 = run_step(x, xa, xold, g, gb, flags, s, eps, a)
    assert np.array_equal(out, out2, equal_nan=True) and np.array_equal(old, old2) and np.array_equal(norms, norms2, equal_nan=True)
    return out, norms


@pytest.mark.parametrize("per", [4, 1028, 3072, 150528])
def test_step_matches_the_float32_restatement_given_the_norms(per):
    """The first step (a = 1, flags NULL, x_adv_old a copy of x_adv) and a later one (a = 0.75, with flags and a RESTORE row), each
    (i) with a large step and a small eps and (ii) with a tiny step and eps = 100.  In (i) the first projection binds in both (n1 > eps);
    the second binds (n2 > eps) at a = 0.75, where the momentum term carries the iterate's distance from x.  At a = 1 the listing gives
    v = xa + (z - xa), which is z up to rounding, and ||z - x|| <= eps already: n2 > eps cannot occur there beyond rounding, so
    n2 <= eps (1 + per 2^-24) + sqrt(per) 2^-22 is asserted instead (the first term bounds ||z - x|| as computed, the second the four
    roundings, each at most 2^-24 on values in [0, 1], that lead from z to d2 in every element).  The result lies in the ball up to the
    rounding of its last add: eps (1 + per 2^-24) + sqrt(per) 2^-24."""
    B = 3
    x, xa, xold, g, gb = step_rows(B, per, 7 + per)
    eps_small = 0.005 * per ** 0.5
    flags = [0, APGD_RESTORE, 3]                                # row 1 steps along grad_best
    for a, fl, old in ((1.0, None, xa.copy()), (0.75, flags, xold)):
        # (i) both projections bind
        s = np.full(B, 50 * eps_small, F32)
        out, norms = check_step(x, xa, old, g, gb, fl, s, eps_small, a)
        print(f"per={per} a={a} (i): eps {eps_small:.4g}, n1 {norms[1].tolist()}, n2 {norms[2].tolist()}")
        assert (norms[1] > eps_small).all()
        if a == 1.0:
            assert (norms[2] <= eps_small * (1 + per * U) + per ** 0.5 * 2.0 ** -22).all()
        else:
            assert (norms[2] > eps_small).all()
        dist = np.sqrt(((out.astype(np.float64) - x) ** 2).sum(axis=1))
        assert (dist <= eps_small * (1 + per * U) + per ** 0.5 * U).all() and out.min() >= 0 and out.max() <= 1
        if fl is not None:                                      # the RESTORE row used grad_best: with grad it lands elsewhere
            plain, _, _ = run_step(x, xa, old, g, gb, [0, 0, 3], s, eps_small, a)
            assert not np.array_equal(plain[1], out[1]) and np.array_equal(plain[[0, 2]], out[[0, 2]])
        # (ii) neither binds
        s = np.full(B, 1e-3, F32)
        out, norms = check_step(x, xa, old, g, gb, fl, s, 100.0, a)
        assert (norms[1] < 100.0).all() and (norms[2] < 100.0).all()
        # per-row step sizes, and a row alone gives the norms it has in the batch
        s = np.array([0.5, 0.125, 2.0], F32)
        out, norms = check_step(x, xa, old, g, gb, fl, s, 0.5, a)
        one = slice(1, 2)
        out1, _, norms1 = run_step(x[one], xa[one], old[one], g[one], gb[one], None if fl is None else fl[one], s[one], 0.5, a)
        assert np.array_equal(norms1[:, 0], norms[:, 1]) and np.array_equal(out1[0], out[1])
    # a NaN in a row's gradient: no gradient step for that row, and a finite result
    gnan = g.copy()
    gnan[2, per // 2] = np.nan
    out, norms = check_step(x, xa, xold, gnan, gb, [0, 0, 0], np.full(B, 0.25, F32), 0.5, 0.75)
    assert np.isnan(norms[0, 2]) and np.isfinite(norms[0, :2]).all() and np.isfinite(norms[1:]).all()
    assert np.isfinite(out).all()
    still = np.full(B, 0.0, F32)                                # the same row with a zero step: the same point
    out0, _, _ = run_step(x, xa, xold, g, gb, [0, 0, 0], still, 0.5, 0.75)
    assert np.array_equal(out0[2], out[2]) and not np.array_equal(out0[0], out[0])


# ---- 3. loop parity ----------------------------------------------------------------------------------------------------------------------------
class HostAPGDL2(HostAPGD):
    """attack_single_run with norm = 'L2' in float32 on the host: HostAPGD's bookkeeping (observe) with the L2 step, fed the GPU's
    logits, gradient, loss and norms of each iteration."""

    def do_step(self, i, norms):
        shape = self.x_adv.shape
        f = lambda t: t.reshape(shape[0], -1).numpy()            # noqa: E731
        out, old, _, _ = l2_step32(f(self.x), f(self.x_adv), f(self.x_adv_old), f(self.grad), self.step.numpy(), float(self.eps),
                                   1.0 if i == 0 else 0.75, norms=norms.cpu().numpy())
        self.x_adv, self.x_adv_old = torch.from_numpy(out).reshape(shape), torch.from_numpy(old).reshape(shape)


def run_parity_l2(vit, x, y, eps, n_iter, monkeypatch, seed=5, restart=0):
    from nested_diffusion_amd import ops
    from nested_diffusion_amd.autoattack import APGDAttack
    atk = APGDAttack(vit, norm="L2", n_iter=n_iter, eps=eps, seed=seed)
    host = HostAPGDL2(x, y, eps, n_iter, atk.schedule)
    index = torch.arange(x.shape[0], device=DEV) + 100
    taken = []                                                    # the norms of every step, in order
    orig = ops.apgd_l2_step
    monkeypatch.setattr(ops, "apgd_l2_step", lambda *a, **k: taken.append(orig(*a, **k)) or taken[-1])

    def same(name, gpu, want, i):
        assert torch.equal(gpu.cpu(), want), (name, i, float((gpu.cpu().double() - want.double()).abs().max()))

    def trace(i, logits, grad, loss, arrays, st):
        if i < 0:
            assert "norms" not in arrays
            start = ops.apgd_l2_random_start(x.to(DEV), index, eps, seed, restart)
            same("start", arrays["x_adv"], start.cpu(), i)
            host.init(arrays["x_adv"], logits, grad, loss)
            return                                              # the first step runs after this call
        if i == 0:
            host.do_step(0, taken[0])
        host.observe(i, logits, grad, loss)
        if i + 1 < n_iter:
            assert len(taken) == i + 2 and arrays["norms"] is taken[-1]
            host.do_step(i + 1, taken[i + 1])
            same("x_adv_old", arrays["x_adv_old"], host.x_adv_old, i)
        same("x_adv", arrays["x_adv"], host.x_adv, i)
        for name in ("x_best", "grad_best", "x_best_adv"):
            same(name, arrays[name], getattr(host, name), i)
        same("step", st.step, host.step, i)
        same("loss_best", st.loss_best, host.loss_best, i)
        same("acc", st.acc.bool(), host.acc, i)

    acc, adv = atk.attack_single_run(x.to(DEV), y.to(DEV), index, restart=restart, trace=trace)
    monkeypatch.undo()
    assert len(taken) == n_iter
    return host, acc, adv


def test_loop_parity_tiny_vit_full_run(tiny, monkeypatch):
    """Every array of every iteration bit for bit, at the first eps of (0.5, 1.0, 2.0) at which both checkpoint branches run: that is
    eps = 1.0 (53 restores, 11 kept checkpoints; at 0.5 all 64 checkpoints restore, and that run is compared bit for bit as well)."""
    x = images(8, 32, 71)
    y = torch.tensor([0, 1, 1, 0, 1, 0, 0, 1])
    seen = []
    for eps in (0.5, 1.0, 2.0):
        host, acc, adv = run_parity_l2(tiny, x, y, eps, 100, monkeypatch)
        assert torch.equal(acc.cpu(), host.acc)
        assert torch.equal(adv.cpu(), host.x_best_adv)
        seen.append((eps, host.restores, host.keeps))
        if host.restores >= 1 and host.keeps >= 1:
            break
    print(f"apgd-l2 tiny B=8 (eps, restores, kept checkpoints): {seen}")
    assert host.restores >= 1 and host.keeps >= 1, seen           # both branches of the checkpoint rule ran


# ---- 4. generate_attack's rows -------------------------------------------------------------------------------------------------------------------
def test_generate_attack_rows(tiny):
    from nested_diffusion_amd.autoattack import APGDAttack
    vit, eps = tiny, 1.0
    x = images(8, 32, 101)
    per = x[0].numel()
    clean = vit.forward(x.to(DEV)).argmax(1).cpu()
    y = clean.clone()
    y[[2, 5]] = 1 - y[[2, 5]]                                     # misclassified from the start
    atk = APGDAttack(vit, norm="L2", eps=eps, n_restarts=2, n_iter=40, seed=1)
    assert atk.attack_type == "APGD" and atk.epsilon == eps
    runs = []
    orig = atk.attack_single_run

    def watched(xx, yy, index, restart=0, trace=None):
        rec = {}

        def tr(i, logits, grad, loss, arrays, st):
            if i < 0:
                rec["start"], rec["st"] = loss.clone(), st
        out = orig(xx, yy, index, restart=restart, trace=tr)
        assert bool((rec["st"].loss_best >= rec["start"]).all())   # the best loss never falls below the start's
        runs.append((restart, index.cpu().tolist()))
        return out

    atk.attack_single_run = watched
    adv, success = atk.generate_attack(x, y, first_image=40)
    assert runs and runs[0] == (0, [40 + b for b in range(8) if b not in (2, 5)])      # the robust rows, keyed on their global index
    adv_c = adv.cpu()
    pred = vit.forward(adv).argmax(1).cpu()
    assert torch.equal(success.cpu(), pred != y)                  # a fresh forward
    changed = (adv_c != x).flatten(1).any(1)
    assert not changed[[2, 5]].any()                              # misclassified at the start: unchanged, bit for bit
    assert not changed[pred == y].any()                           # never fooled: unchanged
    assert bool((pred[changed] != y[changed]).all())
    dist = (adv_c.double() - x.double()).flatten(1).norm(dim=1)
    assert float(dist.max()) <= eps * (1 + per * U)
    assert float(adv.min()) >= 0 and float(adv.max()) <= 1
    print(f"apgd-l2 rows: eps {eps}, {int(changed.sum())} of 6 robust rows fooled over restarts {[r for r, _ in runs]}")
    adv2, success2 = atk.generate_attack(x, y, first_image=40)    # the keyed start: the same call again gives the same bits
    assert torch.equal(adv2, adv) and torch.equal(success2, success)


# ---- 5. strength -----------------------------------------------------------------------------------------------------------------------------------
def test_apgd_l2_fools_at_least_as_many_as_l2pgd(tiny):
    from nested_diffusion_amd.attack import L2Attack
    from nested_diffusion_amd.autoattack import APGDAttack
    """Uniform-noise images all sit at about the same margin of this random ViT (L2PGD fools at most 1 of 16 at eps = 1 and at least 14
    at eps = 2), so the 16 images are graded in brightness, 0.2 to 1: their margins differ and eps = 1 leaves a mixed batch."""
    vit = tiny
    x = (images(16, 32, 101) * torch.linspace(0.2, 1.0, 16).view(16, 1, 1, 1)).to(DEV)
    y = vit.forward(x).argmax(1)                                  # every image starts correctly classified
    counts = {}
    for eps in (0.25, 0.5, 1.0, 2.0):
        _, ok = L2Attack(eps, "L2PGD", vit, seed=1).generate_attack(x, y)
        counts[eps] = int(ok.sum())
        if 4 <= counts[eps] <= 12:
            break
    else:
        pytest.fail(f"L2PGD fools {counts} of 16: no eps of the list leaves a mixed batch")
    _, apgd_ok = APGDAttack(vit, norm="L2", eps=eps, seed=1).generate_attack(x, y)
    print(f"16 images, L2PGD by eps {counts}; at eps {eps}: L2PGD fools {counts[eps]}, APGD-L2 {int(apgd_ok.sum())}")
    assert int(apgd_ok.sum()) >= counts[eps]


# ---- 6. eot_add --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 1028, 2 * 150528])
def test_eot_add_bit_for_bit(n):
    from nested_diffusion_amd import ops
    rng = np.random.default_rng(n)
    a = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(F32)
    g = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(F32)
    acc = torch.from_numpy(a.copy()).to(DEV)
    out = ops.eot_add(acc, torch.from_numpy(g).to(DEV))
    assert out is acc and np.array_equal(acc.cpu().numpy(), a + g)
    acc = torch.from_numpy(a.copy()).to(DEV)
    ops.eot_add(acc, torch.from_numpy(g).to(DEV), 3)
    assert np.array_equal(acc.cpu().numpy(), (a + g) / F32(3.0))
    with pytest.raises(ValueError):
        ops.eot_add(torch.zeros(6, device=DEV), torch.zeros(6, device=DEV))
    with pytest.raises(ValueError):
        ops.eot_add(torch.zeros(8, device=DEV), torch.zeros(4, device=DEV))


# ---- 7. EOTTarget on the ViT ------------------------------------------------------------------------------------------------------------------
def test_eot_target_on_the_vit(tiny):
    from nested_diffusion_amd.eot import EOTTarget
    vit = tiny
    x = images(4, 32, 33).to(DEV)
    y = torch.tensor([0, 1, 1, 0], device=DEV)
    logits, g, loss = vit.input_grad(x, y)
    t = EOTTarget(vit, 3)
    assert t.device == vit.device
    s3, g3, l3 = t.input_grad(x, y)
    gn = g.cpu().numpy()
    assert np.array_equal(g3.cpu().numpy(), ((gn + gn) + gn) / F32(3.0))      # float32, in call order, one true division (numpy's)
    assert torch.equal(s3, logits) and torch.equal(l3, loss)
    assert torch.equal(t.forward(x), vit.forward(x))
    one = EOTTarget(vit, 1).input_grad(x, y)
    assert all(torch.equal(u, v) for u, v in zip(one, (logits, g, loss)))


# ---- 8. EOTTarget on a tiny EnsembleTarget ---------------------------------------------------------------------------------------------------
def test_eot_target_on_the_ensemble_and_apgd_l2_through_it():
    from nested_diffusion_amd.autoattack import APGDAttack
    from nested_diffusion_amd.ensemble_grad import EnsembleTarget
    from nested_diffusion_amd.eot import EOTTarget
    from test_gpu_cond_grad import build_model
    from test_gpu_ensemble_grad import D_IMG, F_DIM, H_DIM, IMG, TAU, config_of, gen
    K, T, B = 2, 4, 3
    cond, _, _ = build_model(2, IMG, (48, 32, 16))
    nets = [ref_cpu.init_cond_model_params(D_IMG, H_DIM, F_DIM, 2, T, seed=60 + k, denoiser=False) for k in range(K)]
    target = EnsembleTarget(cond, nets, config_of(T), mc=2, members=[0, 1], temperature=TAU, seed=4)
    x = torch.rand(B, 3, IMG, IMG, generator=gen(31)).to(DEV)
    y = (torch.arange(B) % 2).to(DEV)
    t = EOTTarget(target, 4)
    assert not hasattr(t, "vit")
    c = target._calls
    P, g, loss = t.input_grad(x, y)
    assert target._calls == c + 4                                 # four draws, four calls
    draws = [target.input_grad(x, y, noise=target.draw_noise(B, counter=c + k)) for k in range(4)]
    gs = [d[1] for d in draws]
    gn = [v.cpu().numpy() for v in gs]
    assert np.array_equal(g.cpu().numpy(), (((gn[0] + gn[1]) + gn[2]) + gn[3]) / F32(4.0))      # float32, in call order
    assert torch.equal(P, draws[3][0]) and torch.equal(loss, draws[3][2])       # the last draw's
    assert not all(torch.equal(gs[0], v) for v in gs[1:])         # the defence is random: the draws differ
    assert target._calls == c + 4                                 # an explicit noise argument leaves the counter alone
    eps = 1.0
    atk = APGDAttack(EOTTarget(target, 2), norm="L2", eps=eps, n_iter=3, n_restarts=1, seed=2)
    c = target._calls
    acc, adv = atk.attack_single_run(x, y, torch.arange(B, device=DEV))
    assert target._calls == c + 2 * 4                             # the start's gradient and three iterations, two draws each
    assert bool(adv.isfinite().all()) and float(adv.min()) >= 0 and float(adv.max()) <= 1
    assert float((adv.double() - x.double()).flatten(1).norm(dim=1).max()) <= eps * (1 + D_IMG * U)
    assert acc.shape == (B,)


# ---- 9. make_attacks --attack_name APGDL2 --eot 2 -------------------------------------------------------------------------------------------
def test_make_attacks_apgdl2_with_eot_end_to_end(tmp_path, capsys, monkeypatch):
    from PIL import Image
    from test_gpu_cli import _write_image_tree, _write_run
    from nested_diffusion_amd import autoattack, make_attacks
    from nested_diffusion_amd.eot import EOTTarget
    tmp = str(tmp_path)
    ypath, *_ = _write_run(tmp, T=6, K=5, B=3, img=224)
    dataroot = os.path.join(tmp, "data")
    _write_image_tree(dataroot)
    out = os.path.join(tmp, "attacked")
    built, returned = [], []
    orig_init = autoattack.APGDAttack.__init__

    def small(self, predict, **kw):                                # the CLI's arguments, then a run short enough for a test
        assert (kw["norm"], kw["n_restarts"], kw["n_iter"], kw["eps"], kw["seed"]) == ("L2", 5, 100, 2.0, 2)
        built.append(predict)
        orig_init(self, predict, **{**kw, "n_iter": 6, "n_restarts": 2})

    monkeypatch.setattr(autoattack.APGDAttack, "__init__", small)
    orig_write = make_attacks.write_attacked_set
    monkeypatch.setattr(make_attacks, "write_attacked_set", lambda *a, **k: returned.append(orig_write(*a, **k)) or returned[-1])
    assert make_attacks.main(["--config", ypath, "--attack_name", "APGDL2", "--eps", "2.0", "--out", out, "--dataroot", dataroot,
                              "--batch_size", "3", "--seed", "2", "--eot", "2"]) == 0
    assert len(built) == 1 and isinstance(built[0], EOTTarget) and built[0].n == 2
    text = capsys.readouterr().out
    assert f"APGDL2 eps=2.0: 7 images written under {os.path.join(out, 'Test_attacks_APGDL2')}, {returned[0]} successful attacks" in text
    tree = os.path.join(out, "Test_attacks_APGDL2")
    src = os.path.join(dataroot, "testing")
    assert sorted(os.listdir(tree)) == ["NORMAL", "PNEUMONIA"]
    for cls in ("NORMAL", "PNEUMONIA"):
        stems = sorted(os.path.splitext(f)[0] for f in os.listdir(os.path.join(src, cls)) if not f.endswith(".txt"))
        assert sorted(os.listdir(os.path.join(tree, cls))) == [s + ".png" for s in stems]
        for s in stems:
            im = Image.open(os.path.join(tree, cls, s + ".png"))
            assert im.mode == "RGB" and im.size == (224, 224)
