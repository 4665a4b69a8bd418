"""Carlini & Wagner's L2 attack on the GPU: the margin gradient (nd_margin_head_bwd, VisionTransformer.input_grad_margin), the passes of
csrc/nd_attack_l2.hip (nd_cw_attack_space, nd_cw_model_space, nd_cw_control, nd_cw_update) and attack.CarliniWagner, against float64
through the CPU oracle and against numpy float32 restatements; make_attacks.write_attacked_set and Diffusion.test_atk with the new
attacks."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import ref_cpu

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = float("inf")
F32 = np.float32


def images(B, img, seed):
    return torch.rand(B, 3, img, img, generator=torch.Generator().manual_seed(seed))


def f64(vp):
    return {k: v.double() for k, v in vp.items()}


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


@pytest.fixture(scope="module")
def tiny():
    from nested_diffusion_amd.mapping import VisionTransformer
    vp = ref_cpu.init_vit_params(embed=128, depth=5, patch=16, img=32, seed=3)
    return VisionTransformer(vp, 2, DEV), f64(vp), 2, 5, 32


@pytest.fixture(scope="module")
def vitb():
    from nested_diffusion_amd.mapping import VisionTransformer
    vp = ref_cpu.init_vit_params(embed=768, depth=12, patch=16, img=224, seed=11)
    return VisionTransformer(vp, 12, DEV), f64(vp), 12, 12, 224


@pytest.fixture(scope="module")
def batch(tiny):
    """The four images of the issue and their clean labels (class 1 for all four)."""
    x0 = images(4, 32, 51)
    labels = tiny[0].forward(x0.to(DEV)).argmax(1).cpu()
    assert labels.tolist() == [1, 1, 1, 1]
    return x0, labels


# ---- the float64 restatement of CarliniWagner's loop (the listing of nested_diffusion_amd/attack.py) -----------------------------------
def margin64(logits, labels, confidence=0.0):
    onehot = torch.nn.functional.one_hot(labels, logits.shape[1]).bool()
    other = logits.masked_fill(onehot, -INF).argmax(1)
    return logits.gather(1, labels[:, None])[:, 0] - logits.gather(1, other[:, None])[:, 0] + confidence, other


def margin_grad64(vp64, x, labels, consts, heads, depth, confidence=0.0):
    """(logits, d/dx sum_b c_b * max(0, margin_b), margin) through the oracle in float64."""
    xx = x.double().cpu().clone().requires_grad_(True)
    logits = ref_cpu.vit_full_forward(vp64, xx, heads, depth)
    margin, _ = margin64(logits, labels.cpu(), confidence)
    (consts.double().cpu() * margin.clamp_min(0)).sum().backward()
    return logits.detach(), xx.grad, margin.detach()


def cw64(vp64, heads, depth, x0, labels, eps, binary_search_steps=6, steps=1000, stepsize=0.01, confidence=0.0, initial_const=1e-3,
         abort_early=True):
    """The listing, in float64 on the host: (adv, best_norm)."""
    x0, labels = x0.double().cpu(), labels.cpu()
    B, a, b = x0.shape[0], 0.5, 0.5
    col = lambda t: t.reshape(-1, 1, 1, 1)                                 # noqa: E731
    w0 = torch.atanh(((x0 - a) / b) * 0.999999)
    xrec = torch.tanh(w0) * b + a
    consts = torch.full((B,), initial_const, dtype=torch.float64)
    lower, upper = torch.zeros(B, dtype=torch.float64), torch.full((B,), INF, dtype=torch.float64)
    best, best_norm = torch.zeros_like(x0), torch.full((B,), INF, dtype=torch.float64)
    for bs in range(binary_search_steps):
        if bs == binary_search_steps - 1 and binary_search_steps >= 10:
            consts = upper.clamp_max(1e10)
        delta, m, v = torch.zeros_like(x0), torch.zeros_like(x0), torch.zeros_like(x0)
        found, prev = torch.zeros(B, dtype=torch.bool), INF
        for k in range(steps):
            t = torch.tanh(w0 + delta)
            x = t * b + a
            logits, dx, margin = margin_grad64(vp64, x, labels, consts, heads, depth, confidence)
            loss = consts * margin.clamp_min(0) + ((x - xrec) ** 2).flatten(1).sum(1)
            g = (dx + 2 * (x - xrec)) * b * (1 - t * t)
            m, v = 0.9 * m + 0.1 * g, 0.999 * v + 0.001 * g * g
            delta = delta - stepsize * (m / (1 - 0.9 ** (k + 1))) / (torch.sqrt(v / (1 - 0.999 ** (k + 1))) + 1e-8)
            if abort_early and k % math.ceil(steps / 10) == 0:
                if not float(loss.sum()) <= 0.9999 * prev:
                    break
                prev = float(loss.sum())
            adv = (logits + confidence * torch.nn.functional.one_hot(labels, logits.shape[1])).argmax(1) != labels
            found |= adv
            norm = (x - x0).flatten(1).norm(dim=1)
            new_best = adv & (norm < best_norm)
            best = torch.where(col(new_best), x, best)
            best_norm = torch.where(new_best, norm, best_norm)
        upper = torch.where(found, consts, upper)
        lower = torch.where(found, lower, consts)
        consts = torch.where(torch.isinf(upper), consts * 10, (lower + upper) / 2)
    p = best - x0
    return x0 + p * col((eps / p.flatten(1).norm(dim=1).clamp_min(1e-12)).clamp_max(1.0)), best_norm


# ---- 1. the margin gradient --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,B", [("tiny", 4), ("vitb", 2)])
def test_input_grad_margin(which, B, request):
    from nested_diffusion_amd import ops
    vit, vp64, heads, depth, img = request.getfixturevalue(which)
    x = images(B, img, 51 if which == "tiny" else 21)
    clean = vit.forward(x.to(DEV))
    labels = clean.argmax(1).cpu()
    labels[1] = (labels[1] + 1) % clean.shape[1]              # row 1 is attacked at a class it does not hold: margin < 0
    consts = torch.tensor([0.5, 2.0, 0.0, 10.0])[:B]
    logits, dx, margin = vit.input_grad_margin(x.to(DEV), labels.to(DEV), consts.to(DEV))
    assert torch.equal(logits, clean)                         # the forward inside is forward(), bit for bit
    _, g_ref, _ = margin_grad64(vp64, x, labels, consts, heads, depth)
    assert (margin.cpu()[[0] + list(range(2, B))] > 0).all() and float(margin[1]) < 0
    r = rel_l2(dx, g_ref)
    m = float((dx.cpu().double() - g_ref).abs().max() / g_ref.abs().max())
    print(f"{which}: margin gradient rel L2 {r:.3e}, max |g - g_ref| / max |g_ref| {m:.3e}")
    assert r <= 1e-4 and m <= 1e-3                            # test_input_grad's bounds for the same chain
    assert not dx[1].any() and bool(dx[0].any())              # a row whose margin is <= 0: dx == 0 exactly
    if B > 2:
        assert not dx[2].any() and bool(dx[3].any())          # and a row whose constant is 0
    # margin and other against the host, on the device's own logits
    l = logits.cpu()
    _, mg, other = ops.margin_head_grad(logits, labels.to(DEV), consts.to(DEV), vit.p["head.weight"], 0.25)
    want_m, want_o = margin64(l, labels, 0.0)
    assert torch.equal(other.cpu().long(), want_o)
    assert torch.equal(margin.cpu(), want_m) and torch.equal(mg.cpu(), want_m + 0.25)
    # the same call again: the same bits
    again = vit.input_grad_margin(x.to(DEV), labels.to(DEV), consts.to(DEV))
    assert torch.equal(again[1], dx) and torch.equal(again[2], margin)


@pytest.mark.parametrize("C", [3, 1024])
def test_margin_head_ties_and_nan(C):
    from nested_diffusion_amd import ops
    g = torch.Generator().manual_seed(C)
    E, B = 96, 6
    logits = torch.randn(B, C, generator=g)
    labels = torch.tensor([0, 1, 2, 0, 1, C - 1])
    logits[0, 1] = logits[0, C - 1] = 9.0                     # a tie among the others: the first index wins
    logits[1, 1] = 20.0                                       # the label holds the maximum: it is excluded
    logits[2, 0] = float("nan")                               # a NaN never wins
    logits[3, 1:] = float("nan")                              # no number among the others: the first non-label column
    logits[3, 0] = 1.0
    logits[4, :] = -5.0                                       # all equal: column 0
    logits[5, C - 1] = -30.0                                  # margin < 0: no gradient
    consts = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    w = torch.randn(C, E, generator=g)
    dfeat, margin, other = ops.margin_head_grad(logits.to(DEV), labels, consts.to(DEV), w.to(DEV), 0.5)
    def first_max_excluding(row, y):                          # the first maximal number among the non-label columns
        arg = None
        for c, v in enumerate(row):
            if c != y and v == v and (arg is None or v > row[arg]):
                arg = c
        return arg if arg is not None else (1 if y == 0 else 0)

    want_o = [first_max_excluding(logits[b].tolist(), int(labels[b])) for b in range(B)]
    assert want_o[0] == 1 and want_o[3] == 1 and want_o[4] == 0 and want_o[2] != 0 and want_o[1] != 1
    assert other.cpu().tolist() == want_o
    want_m = torch.stack([(logits[b, labels[b]] - logits[b, want_o[b]]) + 0.5 for b in range(B)])
    assert torch.equal(margin.cpu()[[0, 1, 2, 4, 5]], want_m[[0, 1, 2, 4, 5]]) and math.isnan(float(margin[3]))
    on = want_m > 0                                           # NaN: off
    assert bool(on[1]) and bool(on[4]) and not bool(on[3]) and not bool(on[5])
    want = torch.stack([consts[b] * (w[labels[b]] - w[want_o[b]]).double() * float(on[b]) for b in range(B)])
    assert float((dfeat.cpu().double() - want).abs().max()) <= 2.0 ** -22 * float(consts.max() * w.abs().max())
    assert not dfeat[3].any() and not dfeat[5].any()
    with pytest.raises(ValueError):
        ops.margin_head_grad(logits.to(DEV), torch.full((B,), C), consts.to(DEV), w.to(DEV))
    # unchecked, an out-of-range label gives a NaN margin and no gradient
    d2, m2, o2 = ops.margin_head_grad(logits.to(DEV), torch.full((B,), C), consts.to(DEV), w.to(DEV), check_labels=False)
    assert torch.isnan(m2).all() and (o2 == -1).all() and not d2.any()


# ---- 2. the transcendental passes ----------------------------------------------------------------------------------------------------------
def test_attack_space_and_model_space():
    """Against float64; the bound is 4 x the error of torch's CPU float32 evaluation of the same formula on the same inputs (the
    device library documents a few ulp, the CPU's <= 1 ulp), floored at 2^-23.  Measured on the MI355X (EXPERIMENTS.md #41), max
    absolute error, device / CPU: w0 6.596e-3 / 6.596e-3, xrec 5.3e-8 / 5.1e-8, t 8.9e-8 / 4.8e-8, x 5.2e-8 / 5.1e-8.  w0's error
    sits at x0 = 0 and 1: the float32 rounding of the argument 0.999999 * (2 x0 - 1), which atanh magnifies by 1 / (1 - y^2) = 5e5
    in either implementation."""
    from nested_diffusion_amd import ops
    B, per = 3, 768
    g = torch.Generator().manual_seed(8)
    x0 = torch.rand(B, per, generator=g)
    x0[0, :4] = torch.tensor([0.0, 1.0, 0.5, 0.25])
    x0[1, :256] = torch.linspace(0, 1, 256)
    x0[2, -4:] = torch.tensor([1.0, 0.0, 1e-7, 1 - 2.0 ** -24])
    w0, xrec = ops.cw_attack_space(x0.to(DEV))
    w64 = torch.atanh(((x0.double() - 0.5) / 0.5) * 0.999999)
    r64 = torch.tanh(w64) * 0.5 + 0.5
    w32 = torch.atanh(((x0 - 0.5) / 0.5) * 0.999999)
    r32 = torch.tanh(w32) * 0.5 + 0.5
    delta = 0.3 * torch.randn(B, per, generator=g)
    delta[0, :4] = 0
    s = ops.CwState(x0.to(DEV))
    s.delta.copy_(delta)
    x = ops.cw_model_space(w0, x0.to(DEV), xrec, s)
    t64 = torch.tanh(w0.cpu().double() + delta.double())      # from the device's own w0
    x64 = t64 * 0.5 + 0.5
    t32 = torch.tanh(w0.cpu() + delta)
    x32 = t32 * 0.5 + 0.5
    assert torch.isfinite(w0).all() and torch.isfinite(s.t).all()
    for name, gpu, cpu, ref in (("w0", w0, w32, w64), ("xrec", xrec, r32, r64), ("t", s.t, t32, t64), ("x", x, x32, x64)):
        e_gpu = float((gpu.cpu().double() - ref).abs().max())
        e_cpu = float((cpu.double() - ref).abs().max())
        bound = max(4 * e_cpu, 2.0 ** -23)                   # the device library documents a few ulp, the CPU's <= 1 ulp
        print(f"{name}: max error against float64: GPU {e_gpu:.3e}, torch CPU float32 {e_cpu:.3e} (bound {bound:.3e})")
        assert e_gpu <= bound, name
    # the sums of squares: the bound of the L2 norms, against the float64 sum over the fp32 differences actually formed
    tol = (per + 1) * 2.0 ** -24
    xn, x0n, rn = x.cpu().numpy(), x0.numpy(), xrec.cpu().numpy()
    for got, diff, name in ((s.sq_rec, xn - rn, "sq_rec"), (s.sq_x0, xn - x0n, "sq_x0")):
        want = (diff.astype(np.float64) ** 2).sum(axis=1)
        rel = np.abs(got.cpu().double().numpy() - want) / want
        print(f"{name}: relative error {rel.max():.3e} (bound {tol:.3e})")
        assert (rel <= tol).all(), name
    # delta = 0 reproduces xrec bit for bit, and the pass is reproducible
    sq = s.sq_rec.clone(), s.sq_x0.clone()
    ops.cw_model_space(w0, x0.to(DEV), xrec, s)
    assert torch.equal(s.sq_rec, sq[0]) and torch.equal(s.sq_x0, sq[1])
    s.delta.zero_()
    assert torch.equal(ops.cw_model_space(w0, x0.to(DEV), xrec, s), xrec) and not s.sq_rec.any()


# ---- 3. nd_cw_update -----------------------------------------------------------------------------------------------------------------------
def adam32(delta, m, v, dx, x, xrec, t, stepsize, k, b_half=0.5):
    bc1, bc2 = F32(1.0 - 0.9 ** (k + 1)), F32(1.0 - 0.999 ** (k + 1))
    g = ((dx + F32(2.0) * (x - xrec)) * F32(b_half)) * (F32(1.0) - t * t)
    m = F32(0.9) * m + F32(0.1) * g
    v = F32(0.999) * v + F32(0.001) * (g * g)
    return delta - (F32(stepsize) * (m / bc1)) / (np.sqrt(v / bc2) + F32(1e-8)), m, v


@pytest.mark.parametrize("per", [4, 3072, 150528])
def test_cw_update(per):
    from nested_diffusion_amd import ops
    B = 3
    g = torch.Generator().manual_seed(per)
    x0 = torch.rand(B, per, generator=g).to(DEV)
    w0, xrec = ops.cw_attack_space(x0)
    s = ops.CwState(x0)
    s.delta.copy_(0.2 * torch.randn(B, per, generator=g))
    assert not s.best.any() and torch.isinf(s.best_norm).all()
    for k, flags in ((0, [1, 0, 1]), (1, [0, 0, 0]), (9, [0, 1, 0])):
        x = ops.cw_model_space(w0, x0, xrec, s).clone()       # the device's own t and x
        dx = (torch.randn(B, per, generator=g) * 10.0 ** (k % 3 - 1)).to(DEV)
        s.flags.copy_(torch.tensor(flags, dtype=torch.int32))
        before = [a.cpu().numpy().copy() for a in (s.delta, s.m, s.v)]
        best_before = s.best.clone()
        ops.cw_update(s, dx, xrec, 0.01, k)
        want = adam32(*before, dx.cpu().numpy(), x.cpu().numpy(), xrec.cpu().numpy(), s.t.cpu().numpy(), 0.01, k)
        for got, w, name in zip((s.delta, s.m, s.v), want, ("delta", "m", "v")):
            assert np.array_equal(got.cpu().numpy(), w), (name, k)
        for b in range(B):                                    # best changes exactly in the flagged rows and takes the pre-update x
            assert torch.equal(s.best[b], x[b] if flags[b] else best_before[b]), (k, b)
        assert torch.equal(s.x, x)
    # a zero gradient leaves delta where it is
    s.reset_search_step()
    assert not s.delta.any() and not s.m.any() and not s.v.any() and not s.found.any()
    x = ops.cw_model_space(w0, x0, xrec, s)
    assert torch.equal(x, xrec)
    ops.cw_update(s, torch.zeros_like(x0), xrec, 0.01, 0, use_flags=False)
    assert not s.delta.any() and not s.m.any() and not s.v.any()


# ---- 4. nd_cw_control ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("confidence", [0.0, 0.5])
def test_cw_control(confidence):
    from nested_diffusion_amd import ops
    nan = float("nan")
    #                   logits               label  best_norm before
    cases = [([2.0, 1.0, 0.0], 0, 5.0),      # not adversarial
             ([1.0, 2.0, 0.0], 0, 5.0),      # adversarial and closer
             ([1.0, 2.0, 0.0], 0, 1.0),      # adversarial and farther
             ([1.0, 1.25, 0.0], 0, 5.0),     # a bare win: adversarial at confidence 0, not at 0.5
             ([nan, nan, nan], 1, 5.0),      # the NaN row: index 0
             ([nan, 3.0, 1.0], 1, INF),      # a NaN never wins: the label holds the maximum
             ([1.0, 1.0, 1.0], 2, INF),      # a tie: the first index, adversarial (at confidence 0)
             ([0.0, 0.0, 4.0], 1, INF)]      # adversarial, the first find
    B = len(cases)
    logits = torch.tensor([c[0] for c in cases])
    labels = torch.tensor([c[1] for c in cases])
    consts = torch.linspace(0.5, 4.0, B)
    sq_x0 = torch.tensor([4.0, 4.0, 4.0, 2.0, 2.0, 2.0, 3.0, 7.0])
    sq_rec = torch.linspace(0.1, 0.8, B)
    margin = torch.tensor([1.0 + confidence, -1.0 + confidence, 0.0, -0.25 + confidence, nan, 2.0, 0.0 + confidence, -4.0])
    s = ops.CwState(torch.zeros(B, 4, device=DEV))
    s.best_norm.copy_(torch.tensor([c[2] for c in cases]))
    s.sq_x0.copy_(sq_x0)
    s.sq_rec.copy_(sq_rec)
    s.found[0] = 1                                            # found is sticky
    loss = ops.cw_control(logits.to(DEV), labels, consts.to(DEV), margin.to(DEV), s, confidence)
    # the host restatement
    l = logits.clone()
    l[torch.arange(B), labels] += confidence
    arg = []
    for row in l.tolist():
        best, a = row[0], 0
        for c in range(1, 3):
            if row[c] > best or (best != best and row[c] == row[c]):
                best, a = row[c], c
        arg.append(a)
    adv = torch.tensor(arg) != labels
    assert adv.tolist() == [False, True, True, confidence == 0.0, True, False, confidence == 0.0, True]
    norm = torch.from_numpy(np.sqrt(sq_x0.numpy()))
    before = torch.tensor([c[2] for c in cases])
    new_best = adv & (norm < before)
    assert s.flags.cpu().bool().tolist() == new_best.tolist()
    assert torch.equal(s.best_norm.cpu(), torch.where(new_best, norm, before))
    assert s.found.cpu().bool().tolist() == (adv | torch.tensor([True] + [False] * (B - 1))).tolist()
    want_loss = consts * torch.where(margin > 0, margin, torch.zeros(B)) + sq_rec
    assert torch.equal(loss.cpu(), want_loss) and loss is s.loss


# ---- 5. the whole attack -------------------------------------------------------------------------------------------------------------------
def clip32(best, x0, eps):
    """The final clip_perturbation in numpy float32, with the device's own norm."""
    from nested_diffusion_amd import ops
    out, _, dn = ops.l2_step(best, x0, None, 0.0, eps, -INF, INF, want_norms=True)
    b, a = best.cpu().numpy().reshape(len(dn), -1), x0.cpu().numpy().reshape(len(dn), -1)
    f = np.minimum(F32(1.0), F32(eps) / np.maximum(dn.cpu().numpy(), F32(1e-12))).reshape(-1, 1)
    want = (a + (b - a) * f).reshape(x0.shape)
    assert np.array_equal(out.cpu().numpy(), want)
    return torch.from_numpy(want)


def test_one_iteration_cases(tiny, batch):
    from nested_diffusion_amd import ops
    from nested_diffusion_amd.attack import CarliniWagner
    vit, vp64, heads, depth, img = tiny
    x0, labels = batch
    x0d = x0.to(DEV)
    atk = CarliniWagner(4.0, vit, binary_search_steps=1, steps=1)
    # labels = the clean argmax: nothing is found, and adv is the clipped step towards the zero image (foolbox's behaviour)
    adv, success = atk.generate_attack(x0d, labels.to(DEV))
    assert torch.isinf(atk.last_best_norm).all()
    assert torch.equal(adv.cpu(), clip32(torch.zeros_like(x0d), x0d, 4.0))
    n0 = x0.double().flatten(1).norm(dim=1)
    assert float((adv.cpu().double() - x0.double() * (1 - 4.0 / n0).reshape(-1, 1, 1, 1)).abs().max()) <= 1e-6
    adv64, bn64 = cw64(vp64, heads, depth, x0, labels, 4.0, binary_search_steps=1, steps=1)
    assert torch.isinf(bn64).all() and float((adv.cpu().double() - adv64).abs().max()) <= 1e-6
    # labels = the other class: every row is adversarial at iteration 0, best = xrec
    wrong = 1 - labels
    adv, success = atk.generate_attack(x0d, wrong.to(DEV))
    _, xrec = ops.cw_attack_space(x0d)
    assert torch.isfinite(atk.last_best_norm).all() and float(atk.last_best_norm.max()) < 1e-4
    assert torch.equal(adv.cpu(), clip32(xrec, x0d, 4.0))
    assert float((adv.cpu().double() - x0.double()).flatten(1).norm(dim=1).max()) < 1e-4
    assert success.all()                                      # adv keeps x0's class, which is not `wrong`
    adv64, bn64 = cw64(vp64, heads, depth, x0, wrong, 4.0, binary_search_steps=1, steps=1)
    assert torch.isfinite(bn64).all() and float((adv.cpu().double() - adv64).abs().max()) <= 1e-6


def test_whole_attack(tiny, batch, monkeypatch):
    from nested_diffusion_amd.attack import CarliniWagner
    vit = tiny[0]
    x0, labels = batch
    per = x0[0].numel()
    reads = []
    orig = CarliniWagner._read_losses
    monkeypatch.setattr(CarliniWagner, "_read_losses", staticmethod(lambda loss: reads.append(tuple(loss.shape)) or orig(loss)))
    atk = CarliniWagner(4.0, vit, binary_search_steps=6, steps=30)
    adv, success = atk.generate_attack(x0.to(DEV), labels.to(DEV))
    # the float64 restatement finds all four rows (best norms 0.99 - 1.72; the first find at constant 1 for one row, 10 for the others)
    print(f"CW: success {success.tolist()}, best norms {atk.last_best_norm.tolist()}, {len(reads)} loss reads")
    assert success.all()
    assert torch.equal(vit.forward(adv).argmax(1).cpu() != labels, success.cpu())
    nrm = (adv.cpu().double() - x0.double()).flatten(1).norm(dim=1)
    assert float(nrm.max()) <= 4.0 * (1 + per * 2.0 ** -24)
    # the only host synchronisation inside a binary-search step: at most 10 reads of B losses
    assert len(reads) <= 10 * 6 and set(reads) == {(4,)}
    adv2, success2 = atk.generate_attack(x0.to(DEV), labels.to(DEV))
    assert torch.equal(adv2, adv) and torch.equal(success2, success)


# ---- 6. make_attacks and test_atk with the new attacks -----------------------------------------------------------------------------------
def _four_image_tree(root):
    from PIL import Image
    rng = np.random.default_rng(17)
    for cls, names in (("NORMAL", ("a.png", "b.png")), ("PNEUMONIA", ("c.png", "d.png"))):
        d = os.path.join(root, "testing", cls)
        os.makedirs(d)
        for name in names:
            Image.fromarray(rng.integers(0, 256, size=(224, 224, 3), dtype=np.uint8), "RGB").save(os.path.join(d, name))


def test_write_attacked_set_and_test_atk(tmp_path, capsys, monkeypatch):
    import types
    import yaml
    from test_gpu_attack_e2e import FLAGS, _run_main
    from test_gpu_cli import _write_run
    import nested_diffusion_amd.runner as runner_mod
    from nested_diffusion_amd import data, make_attacks
    from nested_diffusion_amd import main as nd_main
    from nested_diffusion_amd.attack import CarliniWagner, L2Attack
    tmp = str(tmp_path)
    ypath, *_ = _write_run(tmp, T=6, K=5, B=2, img=224)
    dataroot = os.path.join(tmp, "data")
    _four_image_tree(dataroot)
    out = os.path.join(tmp, "attacked")
    # BIM through the command line
    assert make_attacks.main(["--config", ypath, "--attack_name", "BIM", "--eps", "2.0", "--out", out, "--dataroot", dataroot,
                              "--batch_size", "3"]) == 0
    assert "BIM eps=2.0: 4 images written" in capsys.readouterr().out
    # CW from Python: write_attacked_set with a CarliniWagner
    config = nd_main.dict2namespace(yaml.safe_load(open(ypath)))
    vit = make_attacks.load_vit(config, torch.device(DEV, 0))
    n_ok = make_attacks.write_attacked_set(config, CarliniWagner(2.0, vit, binary_search_steps=1, steps=2), "CW", out,
                                           batch_size=4, dataroot=dataroot)
    assert 0 <= n_ok <= 4 and "CW eps=2.0: 4 images written" in capsys.readouterr().out
    clean = data.ImageFolderDataset(os.path.join(dataroot, "testing"), "ChestXRay", "grayscaled")
    for name in ("BIM", "CW"):
        tree = os.path.join(out, f"Test_attacks_{name}")
        assert sorted(os.listdir(tree)) == ["NORMAL", "PNEUMONIA"]
        assert sorted(os.listdir(os.path.join(tree, "NORMAL"))) == ["a.png", "b.png"]
        cfg = types.SimpleNamespace(data=types.SimpleNamespace(dataset=f"ChestXRayAtk{name}", dataroot=out))
        ds = data.get_dataset(types.SimpleNamespace(preprocess="grayscaled"), cfg)
        assert len(ds) == 4 and ds.classes == ["NORMAL", "PNEUMONIA"]
        for i in range(4):
            (adv, t), (x, t0) = ds[i], clean[i]
            assert t == t0 and adv.shape == (3, 224, 224)
            # inside the L2 ball up to the 8-bit rounding of the PNG (at most 0.5 / 255 per element)
            assert float((adv - x).norm()) <= 2.0 * (1 + 1e-3) + (0.5 / 255) * (3 * 224 * 224) ** 0.5
    # Diffusion.test_atk(attack=L2Attack(...)) runs on one small batch and reports
    items = [clean[i] for i in range(2)]
    batches = [(torch.stack([x for x, _ in items]), torch.tensor([t for _, t in items]))]
    seen = {}
    orig_atk = runner_mod.Diffusion.test_atk

    def spy(self, test_loader=None, attack=None):
        atk = L2Attack(2.0, "L2PGD", self.cond_pred_model, seed=3)
        atk.steps = 3
        orig_atk(self, test_loader=batches, attack=atk)
        seen["report"] = self.last_report
        return orig_atk(self, test_loader=batches)

    monkeypatch.setattr(runner_mod.Diffusion, "test_atk", spy)
    assert _run_main(FLAGS + ["--config", ypath, "--dataroot", dataroot, "--doc", "l2", "--exp", os.path.join(tmp, "r")]) == 0
    assert "Majority voting accuracy for MC:" in capsys.readouterr().out and seen["report"]
