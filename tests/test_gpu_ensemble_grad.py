"""The input gradient through the sampler on the GPU: the kernels of csrc/nd_ensemble_grad.hip against their float64 formulas, one member's
SamplerTape and the whole EnsembleTarget chain against float64 autograd through the oracle (oracle/ref_cpu.py: compute_guiding_prediction,
softmax, ensemble_predict, -log prob[label]), determinism, the gradient attacks pointed at the target, and the refusals.

Tolerance rule of the oracle comparisons: the same oracle is run once more in float32 autograd; e32 = its relative L2 distance to float64.
e32 <= 5e-6 is asserted as a condition on the INPUTS (a chain that amplifies its start is a bad test, not a bad kernel), then the GPU's
rel_l2 against float64 must be <= max(1e-5, 4 e32): 1e-5 is the project's criterion for its other gradient chains, and the factor 4 allows a
different summation order in every contraction plus the BatchNorm fold, each a rounding of the size the fp32 oracle itself commits."""
import types

import pytest
import torch

from oracle import ref_cpu
from test_gpu_attack import f64, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24                       # unit roundoff of fp32: one rounded operation moves a value by at most U relative
E32_MAX = 5e-6
TAU = 0.2555


def gen(seed):
    return torch.Generator().manual_seed(seed)


def f32(p):
    return {k: v.float() for k, v in p.items()}


def tol(e32):
    return max(1e-5, 4 * e32)


# ---- 1. the block's activation backward ------------------------------------------------------------------------------------------------
def act_inputs(B, mc, N, seed):
    """dh, the taped h = softplus(z) (float64 softplus of an fp32 z, rounded once), a_t, mul, and what dmul_acc held before.  z spans
    [-40, 40] and takes -30, +-16, the threshold 20 exactly, its fp32 neighbours and the ends of the range."""
    g = gen(seed)
    M = B * mc
    z = torch.rand(M, N, generator=g) * 80 - 40
    zf = z.view(-1)
    for i, v in enumerate((-30.0, 16.0, -16.0, 20.0, 20.000002, 19.999998, 40.0, -40.0)):
        zf[(7 * i) % zf.numel()] = v
    h = torch.nn.functional.softplus(z.double()).float()
    return (torch.randn(M, N, generator=g), h, torch.rand(N, generator=g) + 0.5, torch.randn(B, N, generator=g), torch.randn(B, N, generator=g))


def act_ref64(dh, h, a, mul, prev, B):
    """The listing of include/nested_diffusion.h in float64 on the same fp32 inputs: (du, dmul_acc, sum_trials |dh h| + |prev|)."""
    dh, a = dh.double(), a.double()
    M, N = dh.shape
    sg = torch.ones_like(dh) if h is None else torch.where(h.double() > 20, torch.ones_like(dh), -torch.expm1(-h.double()))
    g = dh if mul is None else dh * mul.double().repeat(M // B, 1)
    du = g * sg * a
    if mul is None:
        return du, None, None
    terms = (dh * h.double()).reshape(M // B, B, N)
    return du, prev.double() + terms.sum(0), terms.abs().sum(0) + prev.double().abs()


@pytest.mark.parametrize("mc", [1, 3])
@pytest.mark.parametrize("N", [1, 16, 50, 4096])
@pytest.mark.parametrize("B", [1, 5, 33, 128])
def test_cond_act_grad_against_the_float64_formula(B, N, mc):
    """Per element.  du = ((dh * mul) * sg) * a_t: three rounded multiplications (U each) and sg = -expm1f(-h), for which the device
    library documents 3 ulp = 6 U: (1 + U)^3 (1 + 6 U) - 1 < 10 U.  dmul_acc = prev + sum_trials fl(dh * h): one rounding per product,
    one per addition of the mc-term chain, one for the final addition to what the buffer held: (mc + 2) U on sum |dh h| + |prev|.
    M = B * mc rows: M in {1, 5, 33, 128} at mc = 1."""
    from nested_diffusion_amd import ops
    dh, h, a, mul, prev = act_inputs(B, mc, N, 1000 * B + 10 * N + mc)
    d = lambda t: t.to(DEV)                                   # noqa: E731
    du = ops.cond_act_grad(d(dh), d(h), d(a), B).cpu().double()
    want, _, _ = act_ref64(dh, h, a, None, None, B)
    assert bool(((du - want).abs() <= 10 * U * want.abs() + 1e-38).all()), "without mul"
    acc = d(prev).clone()
    du = ops.cond_act_grad(d(dh), d(h), d(a), B, mul=d(mul), dmul_acc=acc).cpu().double()
    want, want_acc, mag = act_ref64(dh, h, a, mul, prev, B)
    assert bool(((du - want).abs() <= 10 * U * want.abs() + 1e-38).all()), "with mul"
    assert bool(((acc.cpu().double() - want_acc).abs() <= (mc + 2) * U * mag + 1e-38).all()), "dmul_acc"
    # no activation (the `norm` layer): du = dh * a_t, one rounding
    du = ops.cond_act_grad(d(dh), None, d(a), B).cpu().double()
    assert bool(((du - dh.double() * a.double()).abs() <= U * (dh.double() * a.double()).abs() + 1e-38).all())
    # the forward's counterpart: one rounded product
    y = ops.cond_mul(d(h), d(mul)).cpu().double()
    ref = h.double() * mul.double().repeat(mc, 1)
    assert bool(((y - ref).abs() <= U * ref.abs() + 1e-45).all())


def test_cond_act_grad_far_below_zero_and_nan_rows():
    from nested_diffusion_amd import ops
    B, mc, N = 3, 2, 16
    dh, h, a, mul, prev = act_inputs(B, mc, N, 5)
    z = torch.full((B * mc,), -30.0)
    h[:, 3] = torch.nn.functional.softplus(z.double()).float()          # 9.4e-14: 1 - exp(-h) is 0 in fp32, -expm1(-h) is not
    dh[:, 3] = 1.0 + torch.arange(B * mc).float()
    assert bool((1.0 - torch.exp(-h[:, 3]) == 0).all())
    acc = prev.to(DEV).clone()
    du = ops.cond_act_grad(dh.to(DEV), h.to(DEV), a.to(DEV), B, mul=mul.to(DEV), dmul_acc=acc).cpu()
    want, _, _ = act_ref64(dh, h, a, mul, prev, B)
    assert bool((du[:, 3] != 0).all()) and bool(((du[:, 3].double() - want[:, 3]).abs() <= 10 * U * want[:, 3].abs()).all())
    # a NaN in row r = 4 (trial 1, image 1) reaches row 4 of du and image 1 of dmul_acc, nothing else
    clean_du, clean_acc = du, acc.cpu()
    bad = dh.clone()
    bad[4, 7] = float("nan")
    acc = prev.to(DEV).clone()
    du = ops.cond_act_grad(bad.to(DEV), h.to(DEV), a.to(DEV), B, mul=mul.to(DEV), dmul_acc=acc).cpu()
    nan_du, nan_acc = torch.zeros(B * mc, N, dtype=torch.bool), torch.zeros(B, N, dtype=torch.bool)
    nan_du[4, 7] = nan_acc[1, 7] = True
    assert torch.equal(du.isnan(), nan_du) and torch.equal(acc.cpu().isnan(), nan_acc)
    assert torch.equal(du[~nan_du], clean_du[~nan_du]) and torch.equal(acc.cpu()[~nan_acc], clean_acc[~nan_acc])


def test_cond_act_grad_refusals():
    from nested_diffusion_amd import _lib, ops
    lib = _lib.load()
    t = lambda *s: torch.ones(*s, device=DEV)                  # noqa: E731
    for kw in (dict(mul=t(2, 8)), dict(dmul_acc=t(2, 8))):     # mul and dmul_acc come together
        with pytest.raises(ValueError):
            ops.cond_act_grad(t(4, 8), t(4, 8), t(8), 2, **kw)
    with pytest.raises(ValueError):
        ops.cond_act_grad(t(5, 8), t(5, 8), t(8), 2)            # M % B != 0
    with pytest.raises(ValueError):
        ops.cond_act_grad(t(4, 8), t(4, 7), t(8), 2)
    with pytest.raises(ValueError):
        ops.cond_act_grad(t(4, 8), None, t(8), 2, mul=t(2, 8), dmul_acc=t(2, 8))     # the product needs the taped h
    out = torch.full((4, 8), 7.0, device=DEV)
    p = lambda x: x.data_ptr()                                 # noqa: E731
    a, b = t(4, 8), t(8)
    assert lib.nd_cond_act_bwd(p(a), p(a), p(b), None, p(out), None, 5, 8, 2, None) != 0
    assert lib.nd_cond_act_bwd(p(a), p(a), p(b), None, p(out), None, 0, 8, 1, None) != 0
    assert lib.nd_cond_act_bwd(p(a), p(a), p(b), None, p(out), None, 4, 0, 2, None) != 0
    assert lib.nd_cond_act_bwd(p(a), p(a), None, None, p(out), None, 4, 8, 2, None) != 0
    assert lib.nd_cond_act_bwd(p(a), p(a), p(b), p(t(2, 8)), p(out), None, 4, 8, 2, None) != 0
    assert lib.nd_cond_mul(p(a), p(t(2, 8)), p(out), 5, 8, 2, None) != 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                            # refused before any launch


# ---- 2. the aggregation head and the softmax backward ------------------------------------------------------------------------------------
def agg64(samples, labels, tau):
    y = samples.double().clone().requires_grad_(True)
    P = ref_cpu.compute_ensemble_confidence(list(y.unbind(0)), tau)
    loss = -torch.log(P[torch.arange(P.shape[0]), labels])
    loss.sum().backward()
    return P.detach(), loss.detach(), y.grad


@pytest.mark.parametrize("tau", [TAU, 1.0])
@pytest.mark.parametrize("S", [1, 6])
def test_aggregate_xent_grad_against_float64_autograd(S, tau):
    """A closed form of a dozen fp32 operations per element on O(1) values: the project's 1e-5 relative L2."""
    from nested_diffusion_amd import ops
    for B in (1, 5):
        for C in (2, 3, 7):
            g = gen(100 * S + 10 * B + C)
            samples = torch.randn(S, B, C, generator=g) * 0.6 + 0.5
            labels = torch.randint(0, C, (B,), generator=g)
            P, loss, d = ops.aggregate_xent_grad(samples.to(DEV), tau, labels.to(DEV))
            P64, loss64, d64 = agg64(samples, labels, tau)
            assert rel_l2(P, P64) <= 1e-5 and rel_l2(loss, loss64) <= 1e-5 and rel_l2(d, d64) <= 1e-5, (S, B, C)
            assert torch.equal(P, ops.aggregate(samples.to(DEV), tau)[0])                 # nd_aggregate's bits
            P_only, no_loss, no_d = ops.aggregate_xent_grad(samples.to(DEV), tau)
            assert no_loss is None and no_d is None and torch.equal(P_only, P)


def test_softmax_grad_against_float64_autograd():
    from nested_diffusion_amd import ops
    for K, B, C in ((1, 1, 2), (3, 5, 3), (5, 4, 7), (2, 3, 1000)):
        g = gen(K + B + C)
        logits, dp = torch.randn(K, B, C, generator=g) * 2, torch.randn(K, B, C, generator=g)
        l64 = logits.double().requires_grad_(True)
        (torch.softmax(l64, dim=2) * dp.double()).sum().backward()
        p = ops.softmax_rows(logits.to(DEV))
        assert rel_l2(ops.softmax_grad(p, dp.to(DEV)), l64.grad) <= 1e-5, (K, B, C)


def test_aggregate_xent_grad_conventions_and_refusals():
    from nested_diffusion_amd import _lib, ops
    S, B, C = 4, 4, 3
    samples = torch.randn(S, B, C, generator=gen(3)) * 0.5 + 0.5
    labels = torch.tensor([0, 1, 2, 0])
    clean = ops.aggregate_xent_grad(samples.to(DEV), TAU, labels.to(DEV))
    rest = lambda got, rows: all(torch.equal(got[0][b], clean[0][b]) and torch.equal(got[1][b], clean[1][b])       # noqa: E731
                                 and torch.equal(got[2][:, b], clean[2][:, b]) for b in rows)
    # P[b, y] == 0: every sample's probability at the label underflows: loss +inf, no gradient
    under = samples.clone()
    under[:, 1, 1] = 13.0                                      # -(12^2) / 0.2555 is 560 below the row's largest logit
    got = ops.aggregate_xent_grad(under.to(DEV), TAU, labels.to(DEV))
    assert float(got[1][1]) == float("inf") and bool((got[2][:, 1] == 0).all()) and float(got[0][1, 1]) == 0.0 and rest(got, (0, 2, 3))
    # a NaN in one of an image's samples: that image's row of P, its loss and all its gradients are NaN
    nan = samples.clone()
    nan[2, 2, 0] = float("nan")
    got = ops.aggregate_xent_grad(nan.to(DEV), TAU, labels.to(DEV))
    assert bool(got[0][2].isnan().all()) and bool(got[1][2].isnan()) and bool(got[2][:, 2].isnan().all()) and rest(got, (0, 1, 3))
    # a label outside [0, C): refused by the wrapper; with check_labels=False the kernel gives loss NaN, gradient 0 and P as usual
    bad = torch.tensor([0, 1, C, -1])
    with pytest.raises(ValueError, match="labels"):
        ops.aggregate_xent_grad(samples.to(DEV), TAU, bad.to(DEV))
    got = ops.aggregate_xent_grad(samples.to(DEV), TAU, bad.to(DEV), check_labels=False)
    assert bool(got[1][2:].isnan().all()) and bool((got[2][:, 2:] == 0).all()) and torch.equal(got[0], clean[0])
    assert torch.equal(got[1][:2], clean[1][:2]) and torch.equal(got[2][:, :2], clean[2][:, :2])
    for shape in ((2, 3, 17), (2, 3), (0, 3, 2)):
        with pytest.raises(ValueError):
            ops.aggregate_xent_grad(torch.zeros(shape, device=DEV), TAU)
    with pytest.raises(ValueError, match="temperature"):
        ops.aggregate_xent_grad(samples.to(DEV), 0.0)
    with pytest.raises(ValueError):
        ops.softmax_grad(torch.zeros(2, 3, device=DEV), torch.zeros(2, 4, device=DEV))
    lib, p = _lib.load(), (lambda x: x.data_ptr())
    z, out, lab = torch.zeros(2, 3, 4, device=DEV), torch.full((2, 3, 4), 7.0, device=DEV), torch.zeros(3, dtype=torch.int64, device=DEV)
    assert lib.nd_aggregate_xent_bwd(p(z), None, p(out), None, None, 2, 3, 17, 1.0, None) != 0
    assert lib.nd_aggregate_xent_bwd(p(z), None, p(out), None, None, 0, 3, 4, 1.0, None) != 0
    assert lib.nd_aggregate_xent_bwd(p(z), None, p(out), None, None, 2, 3, 4, 0.0, None) != 0
    assert lib.nd_aggregate_xent_bwd(p(z), p(lab), p(out), None, None, 2, 3, 4, 1.0, None) != 0       # labels need loss and dsamples
    assert lib.nd_aggregate_xent_bwd(p(z), p(lab), p(out), p(out), p(z), 2, 3, 4, 1.0, None) != 0      # dsamples is samples
    assert lib.nd_softmax_bwd(p(z), p(z), p(out), 0, 4, None) != 0 and lib.nd_softmax_bwd(p(z), p(z), p(z), 6, 4, None) != 0
    assert lib.nd_reverse_step(3, p(z), 4, p(z), p(z), p(z), p(out), 4, 6, 3, 4, 1.0, 0.5, 0.5, None) != 0      # unknown mode
    assert lib.nd_reverse_step(1, p(z), 4, p(z), p(z), p(z), p(out), 4, 6, 3, 9, 1.0, 0.5, 0.5, None) != 0      # C > 8
    assert lib.nd_reverse_step(1, p(z), 4, p(z), p(z), p(z), p(out), 6, 6, 3, 4, 1.0, 0.5, 0.5, None) != 0      # C < ldo < 2C
    assert lib.nd_reverse_step(1, p(z), 4, p(z), p(z), None, p(out), 4, 6, 3, 4, 1.0, 0.5, 0.5, None) != 0      # p_sample needs z
    assert lib.nd_reverse_step_bwd(p(z), 4, 1.0, 1.0, 1.0, None, None, 4, p(out), 7, 3, 4, None) != 0           # M % B != 0
    assert lib.nd_reverse_step_bwd(p(z), 6, 1.0, 1.0, 1.0, None, None, 4, p(out), 6, 3, 4, None) != 0           # C < ldg < 2C
    assert lib.nd_reverse_step_bwd(p(z), 4, 1.0, 1.0, 1.0, None, None, 4, p(z), 6, 3, 4, None) != 0             # dymean is g
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                            # refused before any launch


# ---- 3. one member, sampler only ---------------------------------------------------------------------------------------------------------
def member_oracle(p, x_flat, yhat, noise, cot, alphas, omabs, T, mc, dtype):
    """(y0, dx_flat, dyhat) of L = (y0 * cot).sum() by autograd through ref_cpu.p_sample_loop on rows r = trial * B + image."""
    c = lambda t: t.to(dtype)                                  # noqa: E731
    x, yh = c(x_flat).clone().requires_grad_(True), c(yhat).clone().requires_grad_(True)
    pp = {k: c(v) for k, v in p.items() if v.is_floating_point()}
    y0 = ref_cpu.p_sample_loop(pp, x.repeat(mc, 1), yh.repeat(mc, 1), yh.repeat(mc, 1), T, c(alphas), c(omabs), c(noise))
    (y0 * c(cot)).sum().backward()
    return y0.detach(), x.grad, yh.grad


def check_member(p, T, B, mc, C, D, seed, record_property=None, tag=""):
    from nested_diffusion_amd.ensemble_grad import SamplerTape
    g = gen(seed)
    alphas, omabs = ref_cpu.schedule_tables("linear", T, 1e-4, 0.02)
    x = torch.rand(B, D, generator=g)
    yhat = torch.softmax(torch.randn(B, C, generator=g), dim=1)
    noise, cot = torch.randn(T, B * mc, C, generator=g), torch.randn(B * mc, C, generator=g)
    ref = member_oracle(p, x, yhat, noise, cot, alphas, omabs, T, mc, torch.float64)
    r32 = member_oracle(p, x, yhat, noise, cot, alphas, omabs, T, mc, torch.float32)
    tape = SamplerTape(p, alphas, omabs, DEV)
    y0 = tape.forward(x.to(DEV), yhat.to(DEV), noise.to(DEV))
    dx, dyhat = tape.backward(cot.to(DEV))
    for name, got, want, w32 in zip(("y0", "dx_flat", "dyhat"), (y0, dx, dyhat), ref, r32):
        e32, r = rel_l2(w32, want), rel_l2(got, want)
        print(f"{tag} T={T} B={B} mc={mc} C={C} {name}: e32 {e32:.3e} gpu {r:.3e}")
        if record_property is not None:
            record_property(f"{tag}{name}_T{T}_B{B}_mc{mc}_C{C}", {"e32": e32, "gpu": r})
        assert e32 <= E32_MAX, (name, "the inputs are ill-conditioned", e32)
        assert r <= tol(e32), (name, T, B, mc, C, r, e32)
    with pytest.raises(RuntimeError):                          # a tape serves one backward
        tape.backward(cot.to(DEV))
    return tape


@pytest.mark.parametrize("T", [1, 2, 4])
@pytest.mark.parametrize("C", [2, 3])
def test_one_member_against_the_float64_oracle(T, C, record_property):
    D, H, F = 64, 32, 48
    p = ref_cpu.init_cond_model_params(D, H, F, C, T, seed=40 + C)
    for mc in (1, 3):
        for B in (1, 3):
            check_member(p, T, B, mc, C, D, 7 * T + 3 * mc + B, record_property)


def test_one_member_at_the_real_width(record_property):
    """H = F = 4096 (the config's), D = 256, B = 32, mc = 1, T = 2: every F-wide kernel at its real row length, the 4096-deep
    contractions of nd_linear_bwd.  (The 150528-deep encoder stream has its own real-shape test in test_gpu_cond_grad.py.)"""
    p = ref_cpu.init_cond_model_params(256, 4096, 4096, 2, 2, seed=9)
    check_member(p, 2, 32, 1, 2, 256, 77, record_property, tag="real_width_")


# ---- 4. the whole chain ------------------------------------------------------------------------------------------------------------------
K, MC, B_IMG, IMG = 3, 2, 3, 32
D_IMG, H_DIM, F_DIM = 3 * IMG * IMG, 32, 48
CASES = {"T1": (1, False), "T4": (4, False), "T12_denoiser": (12, True)}


def config_of(T, C=2):
    ns = types.SimpleNamespace
    return ns(data=ns(dataset="ChestXRay", num_classes=C), model=ns(data_dim=D_IMG, hidden_dim=H_DIM, feature_dim=F_DIM),
              diffusion=ns(timesteps=T, beta_schedule="linear", beta_start=1e-4, beta_end=0.02))


@pytest.fixture(scope="module")
def cond_model():
    from test_gpu_cond_grad import build_model
    return build_model(2, IMG, (48, 32, 16))


def chain_oracle(vp, mlps, nets, x, labels, noise, T, members, dtype):
    """(P, loss, dx) by autograd through the oracle: compute_guiding_prediction(full_vit=False), softmax, ensemble_predict,
    -log prob[label], .sum().backward().  noise [len(members), T, B * mc, C], rows r = trial * B + image."""
    c = lambda t: t.to(dtype)                                  # noqa: E731
    cp = lambda p: {k: c(v) for k, v in p.items() if v.is_floating_point()}     # noqa: E731
    alphas, omabs = ref_cpu.schedule_tables("linear", T, 1e-4, 0.02)
    xx = c(x).clone().requires_grad_(True)
    outs = ref_cpu.compute_guiding_prediction(cp(vp), [cp(m) for m in mlps], xx, 2, 3, full_vit=False)
    yhat = [torch.softmax(outs[k], dim=1) for k in members]
    B = x.shape[0]
    nz = c(noise).reshape(len(members), T, MC, B, -1).permute(0, 2, 1, 3, 4)
    _, _, prob = ref_cpu.ensemble_predict([cp(nets[k]) for k in members], xx.reshape(B, -1), yhat, T, c(alphas), c(omabs), nz, TAU)
    loss = -torch.log(prob[torch.arange(B), labels])
    loss.sum().backward()
    return prob.detach(), loss.detach(), xx.grad


@pytest.fixture(scope="module")
def chains(cond_model):
    """Per case: the nets, the target, the inputs and the float64 / float32 oracle results for all members, computed once."""
    from nested_diffusion_amd.ensemble_grad import EnsembleTarget
    cond, vp, mlps = cond_model
    out = {}
    for name, (T, denoiser) in CASES.items():
        nets = [ref_cpu.init_cond_model_params(D_IMG, H_DIM, F_DIM, 2, T, seed=60 + k, denoiser=denoiser) for k in range(K)]
        x = torch.rand(B_IMG, 3, IMG, IMG, generator=gen(31))
        labels = torch.arange(B_IMG) % 2
        noise = torch.randn(K, T, B_IMG * MC, 2, generator=gen(32 + T))
        target = EnsembleTarget(cond, nets, config_of(T), mc=MC, temperature=TAU, seed=4)
        out[name] = dict(T=T, nets=nets, x=x, labels=labels, noise=noise, target=target,
                         ref=chain_oracle(vp, mlps, nets, x, labels, noise, T, [0, 1, 2], torch.float64),
                         r32=chain_oracle(vp, mlps, nets, x, labels, noise, T, [0, 1, 2], torch.float32))
    return out


def compare_chain(got, ref, r32, record_property, tag):
    for name, g, want, w32 in zip(("P", "dx", "loss"), got, ref, r32):
        e32, r = rel_l2(w32, want), rel_l2(g, want)
        print(f"{tag} {name}: e32 {e32:.3e} gpu {r:.3e}")
        record_property(f"{tag}_{name}", {"e32": e32, "gpu": r})
        assert e32 <= E32_MAX, (name, "the inputs are ill-conditioned", e32)
        assert r <= tol(e32), (tag, name, r, e32)


@pytest.mark.parametrize("case", list(CASES))
def test_whole_chain_against_float64_autograd(case, chains, record_property):
    c = chains[case]
    x, labels, noise = c["x"].to(DEV), c["labels"].to(DEV), c["noise"].to(DEV)
    P, dx, loss = c["target"].input_grad(x, labels, noise=noise)
    assert dx.shape == x.shape and bool(dx.isfinite().all())
    ref, r32 = c["ref"], c["r32"]
    compare_chain((P, dx, loss), (ref[0], ref[2], ref[1]), (r32[0], r32[2], r32[1]), record_property, case)
    assert torch.equal(c["target"].forward(x, noise=noise), P)            # the scores-only call forms the same P


@pytest.mark.parametrize("members", [[0, 2], [1]])
def test_whole_chain_member_subsets(members, cond_model, chains, record_property):
    from nested_diffusion_amd.ensemble_grad import EnsembleTarget
    cond, vp, mlps = cond_model
    c = chains["T4"]
    T, noise = c["T"], c["noise"][members].contiguous()
    target = EnsembleTarget(cond, c["nets"], config_of(T), mc=MC, members=members, temperature=TAU)
    P, dx, loss = target.input_grad(c["x"].to(DEV), c["labels"].to(DEV), noise=noise.to(DEV))
    ref = chain_oracle(vp, mlps, c["nets"], c["x"], c["labels"], noise, T, members, torch.float64)
    r32 = chain_oracle(vp, mlps, c["nets"], c["x"], c["labels"], noise, T, members, torch.float32)
    compare_chain((P, dx, loss), (ref[0], ref[2], ref[1]), (r32[0], r32[2], r32[1]), record_property, "members_" + "_".join(map(str, members)))


def test_determinism_and_fresh_noise(chains):
    c = chains["T4"]
    t, x, labels, noise = c["target"], c["x"].to(DEV), c["labels"].to(DEV), c["noise"].to(DEV)
    a, b = t.input_grad(x, labels, noise=noise), t.input_grad(x, labels, noise=noise)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    t.free_noise()
    p1, p2 = t.input_grad(x, labels)[0], t.input_grad(x, labels)[0]       # noise=None: the call counter advances
    assert not torch.equal(p1, p2)
    pinned = t.fix_noise(B=x.shape[0])
    assert tuple(pinned.shape) == (K, c["T"], B_IMG * MC, 2)
    assert torch.equal(t.input_grad(x, labels)[0], t.input_grad(x, labels)[0]) and torch.equal(t(x), t(x))
    t.free_noise()


# ---- 5. attacks on the target ---------------------------------------------------------------------------------------------------------------
EPS = 8 / 255


@pytest.fixture(scope="module")
def attacked(chains):
    """The T = 4 target on one pinned sample path, six images, labelled with the target's own clean predictions: no row starts fooled."""
    t = chains["T4"]["target"]
    x = torch.rand(6, 3, IMG, IMG, generator=gen(5))
    t.fix_noise(B=6)
    labels = t(x.to(DEV)).argmax(dim=1)
    loss0 = t.input_grad(x.to(DEV), labels)[2]
    yield t, x, labels, loss0
    t.free_noise()


def in_ball_and_loss_rises(t, x, labels, loss0, adv, eps, l2):
    d = adv.cpu() - x
    if l2:
        assert float(d.flatten(1).norm(dim=1).max()) <= eps * (1 + 1e-5)
    else:
        assert float(d.abs().max()) <= eps * (1 + 1e-6)
    assert float(adv.min()) >= 0 and float(adv.max()) <= 1
    loss1 = t.input_grad(adv, labels)[2]
    print("loss rise per row:", (loss1 - loss0).cpu().tolist())
    assert bool((loss1 > loss0).all())


def test_fgsm_and_pgd_on_the_target(attacked):
    from nested_diffusion_amd.attack import Attack
    t, x, labels, loss0 = attacked
    for name in ("FGSM", "PGD"):
        atk = Attack(EPS, name, t, seed=3)
        assert atk.model is t
        adv, success = atk.generate_attack(x.to(DEV), labels)
        in_ball_and_loss_rises(t, x, labels, loss0, adv, EPS, False)
        assert torch.equal(success, t(adv).argmax(dim=1) != labels)


def test_l2pgd_on_the_target(attacked):
    from nested_diffusion_amd.attack import L2Attack
    t, x, labels, loss0 = attacked
    adv, _ = L2Attack(2.0, "L2PGD", t, seed=3).generate_attack(x.to(DEV), labels)
    in_ball_and_loss_rises(t, x, labels, loss0, adv, 2.0, True)


def test_apgd_ce_on_the_target(attacked):
    """attack_single_run's highest-loss iterate x_best (AutoAttack itself hands back only the rows it fooled)."""
    from nested_diffusion_amd.autoattack import APGDAttack, AutoAttack
    t, x, labels, loss0 = attacked
    assert AutoAttack(t, eps=EPS, version="custom", attacks_to_run=["apgd-ce"]).model is t
    last = {}
    APGDAttack(t, n_iter=20, eps=EPS, seed=1).attack_single_run(x.to(DEV), labels, torch.arange(6, device=DEV),
                                                                 trace=lambda i, lg, gr, ls, arrays, st: last.update(arrays))
    in_ball_and_loss_rises(t, x, labels, loss0, last["x_best"], EPS, False)


def test_cw_on_the_target_refuses(attacked):
    from nested_diffusion_amd.attack import CarliniWagner
    with pytest.raises(NotImplementedError, match="Carlini"):
        CarliniWagner(0.5, attacked[0])


def test_test_atk_and_write_attacked_set_take_the_target(cond_model, chains, tmp_path, monkeypatch):
    from nested_diffusion_amd import make_attacks
    from nested_diffusion_amd.attack import Attack
    from nested_diffusion_amd.runner import Diffusion
    cond, vp, mlps = cond_model
    T = 4
    cfg = config_of(T)
    cfg.testing = types.SimpleNamespace(batch_size=4)
    cfg.diffusion.aux_cls = types.SimpleNamespace(arch="sevit")
    args = types.SimpleNamespace(seed=1, mc_trials=2, attack_name=None)
    d = Diffusion(args, cfg, device=torch.device(DEV), conditioner=cond, noise_estimator_states=chains["T4"]["nets"])
    target = d.ensemble_target(mc=2)
    assert target.members == [0, 1, 2] and target.temperature == d.temperature and not hasattr(target, "vit")
    loader = [(torch.rand(4, 3, IMG, IMG, generator=gen(8)), torch.tensor([0, 1, 0, 1])) for _ in range(2)]
    acc = d.test_atk(test_loader=loader, attack=Attack(EPS, "FGSM", target))
    assert 0.0 <= float(acc) <= 1.0 and tuple(d.last_probs.shape) == (8, 2)
    with pytest.raises(RuntimeError, match="before"):                     # the injected states are gone once the engine holds them
        d.ensemble_target()

    class Folder:                                                         # what data.get_dataset hands write_attacked_set
        classes = ["a", "b"]
        samples = [(f"/x/img{i}.png", i % 2) for i in range(5)]

        def __len__(self):
            return 5

        def __getitem__(self, i):
            return torch.rand(3, IMG, IMG, generator=gen(90 + i)), i % 2
    import nested_diffusion_amd.data as data
    monkeypatch.setattr(data, "get_dataset", lambda a, c: Folder())
    n_ok = make_attacks.write_attacked_set(cfg, Attack(EPS, "FGSM", target), "FGSM", str(tmp_path), batch_size=3)
    files = sorted(p.relative_to(tmp_path).as_posix() for p in tmp_path.rglob("*.png"))
    assert 0 <= n_ok <= 5 and files == sorted(f"Test_attacks_FGSM/{'ab'[i % 2]}/img{i}.png" for i in range(5))


# ---- 6. refusals, each before any launch --------------------------------------------------------------------------------------------------
def test_target_refusals(cond_model, chains, monkeypatch):
    from nested_diffusion_amd import _lib
    from nested_diffusion_amd.ensemble_grad import EnsembleTarget
    from nested_diffusion_amd.mapping import Classifier, GuidingConditioner, VisionTransformer
    cond, vp, mlps = cond_model
    c = chains["T4"]
    t, x, labels = c["target"], c["x"].to(DEV), c["labels"].to(DEV)
    with pytest.raises(ValueError, match="noise"):
        t.input_grad(x, labels, noise=c["noise"][:, :, :3].to(DEV))
    with pytest.raises(ValueError, match="noise"):
        t.forward(x, noise=c["noise"][:2].to(DEV))
    with pytest.raises(ValueError, match="128"):                          # B * mc = 130
        t.input_grad(torch.rand(65, 3, IMG, IMG, device=DEV), torch.zeros(65, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="labels"):
        t.input_grad(x, labels + 2, noise=c["noise"].to(DEV))
    with pytest.raises(ValueError):
        t.input_grad(torch.rand(3, 3, 16, 16, device=DEV), labels)
    vp16 = ref_cpu.init_vit_params(embed=128, depth=1, patch=16, img=IMG, num_classes=2, seed=3)
    m16 = ref_cpu.init_classifier_params(4 * 128, (64, 32, 32), 2, seed=10)
    cond16 = GuidingConditioner(VisionTransformer(vp16, 2, DEV, "f16"), [Classifier(m16, DEV, "f16")])
    with pytest.raises(_lib.NdError, match="fp16"):
        EnsembleTarget(cond16, c["nets"][:1], config_of(4), temperature=TAU)
    monkeypatch.setenv("ND_GEMM_F32", "mfma_f32")
    with pytest.raises(_lib.NdError, match="mfma_f32"):
        EnsembleTarget(cond, c["nets"], config_of(4), temperature=TAU)
