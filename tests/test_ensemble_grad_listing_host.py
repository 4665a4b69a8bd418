"""The float32 restatements of tests/_ensemble_grad_listing.py against something independent of them, on the CPU: exact rational arithmetic
for the fused multiply-add, float64 autograd through the oracle (oracle/ref_cpu.py p_sample_given_eps, p_sample_t_1to0_given_eps) and
through torch.softmax / softplus, and ensemble_grad.reverse_step_coefficients for the backward's three coefficients.

Yardstick: a listing of n_ops rounded operations differs from its exact value by at most n_ops * U * sum |terms| (U = 2^-24; first order,
each operation's rounding carried to the output through the magnitudes of the terms it feeds).  n_ops is counted from the listing and
written next to each assertion.  The posterior's coefficients cancel at small t in the reference's own fp32 arithmetic (gamma_2 =
1 + (sab_t - 1) (..) / s_t^2), so there 4 |ref_cpu fp32 - float64| is added: posterior64 / assert_stage of tests/test_gpu_step_edges.py,
the rule the step kernels' tests use for the same device function, on the CPU here."""
import random
from fractions import Fraction

import numpy as np
import pytest
import torch

import _ensemble_grad_listing as L
import test_gpu_step_edges as step_edges
from oracle import ref_cpu

U = L.U
T = 1000
TS = (1, 2, 500, 999)
needs_fmaf = pytest.mark.skipif(not L.HAVE_FMAF, reason=L.FMAF_MISSING)


def gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.fixture(scope="module")
def tables():
    return ref_cpu.schedule_tables("linear", T, 1e-4, 0.02)


@pytest.fixture()
def cpu_step_edges(monkeypatch):
    """posterior64 places its fp32 oracle value on test_gpu_step_edges.DEV: the CPU here."""
    monkeypatch.setattr(step_edges, "DEV", "cpu")
    return step_edges


# ---- fmaf -------------------------------------------------------------------------------------------------------------------------------
def round_f32(x):
    """The float32 nearest a Fraction, ties to even, as a Python float (normal and subnormal range; no overflow in these cases)."""
    if x == 0:
        return 0.0
    a, e = abs(x), 0
    while a >= 2 ** (e + 1):
        e += 1
    while a < 2 ** e:
        e -= 1
    q = Fraction(2) ** (max(e, -126) - 23)
    return float(round(x / q) * q)               # round(Fraction) goes to the even integer on a tie; the product is exact in float64


def halfway_cases(n, rng):
    """(a, b, c) whose exact a * b + c lies 2^-70-ish off the midpoint of two float32 neighbours of c: a * b = 2^-24 (1 - k^2 2^-46),
    c = +-(1 + m 2^-23) with m odd.  Rounding the sum to float64 first lands ON the midpoint and then goes to the even neighbour: wrong."""
    out = []
    for _ in range(n):
        k, m = rng.randrange(1, 200), 2 * rng.randrange(0, 2 ** 22) + 1
        a, b = 2.0 ** -24 * (1 + k * 2.0 ** -23), 1 - k * 2.0 ** -23
        out.append((a, b, rng.choice((1.0, -1.0)) * (1 + m * 2.0 ** -23)))
    return out


@needs_fmaf
def test_fmaf_is_correctly_rounded():
    rng = random.Random(5)
    f32 = lambda v: float(np.float32(v))                        # noqa: E731
    cases = [(f32(rng.gauss(0, 1)), f32(rng.gauss(0, 1)), f32(rng.gauss(0, 1))) for _ in range(200)]
    cases += [(f32(rng.gauss(0, 1) * 2.0 ** rng.randrange(-60, 60)), f32(rng.gauss(0, 1) * 2.0 ** rng.randrange(-60, 60)),
               f32(rng.gauss(0, 1) * 2.0 ** rng.randrange(-120, 100))) for _ in range(100)]
    cases += [(x, y, -f32(x * y)) for x, y, _ in cases[:100]]                        # the sum cancels to the product's rounding error
    cases += [(f32(2.0 ** -70 * rng.gauss(0, 1)), f32(2.0 ** -70 * rng.gauss(0, 1)), f32(2.0 ** -140 * rng.gauss(0, 1))) for _ in range(50)]
    hard = halfway_cases(100, rng)
    a, b, c = (np.array(v, dtype=np.float32) for v in zip(*(cases + hard)))
    assert all(float(np.float32(v)) == v for t in cases + hard for v in t)           # every operand is a float32
    got = L.fmaf(a, b, c)
    want = np.array([round_f32(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in cases + hard], dtype=np.float64)
    assert np.array_equal(got.astype(np.float64), want)
    via64 = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32).astype(np.float64)
    n_hard = int((via64[-len(hard):] != want[-len(hard):]).sum())
    print(f"fmaf: {len(want)} cases exact; rounding through float64 first is wrong on {n_hard} of the {len(hard)} midpoint cases")
    assert n_hard == len(hard)                                                       # the cases tell the two apart
    assert np.array_equal(L.fmaf(np.float32(2.0), a[:5], np.float32(0.0)), np.float32(2.0) * a[:5])      # scalars broadcast


# ---- the reverse step -------------------------------------------------------------------------------------------------------------------
def step_inputs(B, mc, C, ldy, seed):
    g = gen(seed)
    M = B * mc
    return dict(y=torch.randn(M, ldy, generator=g), ymean=torch.softmax(torch.randn(B, C, generator=g), -1),
                eps=torch.randn(M, C, generator=g), z=torch.randn(M, C, generator=g))


N_OPS_POSTERIOR = 35      # coefficients: sab_t 3, sab_tm1 3, sa 1, g0 3, g1 2, g2 5, bh 3; y0r 7; mean 5; sqrt(bh) z and the last sum 3
N_OPS_LAST = 10           # sab_t 3, y0r 7
SHAPES = [(1, 1, 1, 1, 1), (1, 1, 1, 2, 64), (3, 2, 2, 16, 16), (7, 1, 5, 10, 9), (5, 3, 3, 7, 5), (33, 2, 8, 64, 64)]


@pytest.mark.parametrize("shape", SHAPES)
def test_reverse_step_listing_against_float64(shape, tables, cpu_step_edges):
    B, mc, C, ldo, ldy = shape
    alphas, omabs = tables
    io = step_inputs(B, mc, C, ldy, 100 * B + C)
    M = B * mc
    rows = torch.arange(M) % B
    y, ym, eps, z = io["y"][:, :C], io["ymean"][rows], io["eps"], io["z"]
    zero = torch.zeros(M, C, dtype=torch.float64)
    n = {k: v.numpy() for k, v in io.items()}

    def layout_ok(out):
        assert out.shape == (M, ldo) and out.dtype == np.float32
        if ldo >= 2 * C:
            assert np.array_equal(out[:, C:2 * C], ym.numpy()) and not out[:, 2 * C:].any() and not np.signbit(out[:, 2 * C:]).any()

    out = L.reverse_step_f32(L.RSTEP_INIT, None, n["ymean"], None, n["z"], 1.0, 0.0, 0.0, ldo)
    layout_ok(out)
    assert np.array_equal(out[:, :C], (z + ym).numpy())                              # one operation: torch's fp32 sum has the same bits
    for t in TS:
        a, s, s1 = float(alphas[t]), float(omabs[t]), float(omabs[t - 1])
        out = L.reverse_step_f32(L.RSTEP_UPDATE, n["y"], n["ymean"], n["eps"], n["z"], a, s, s1, ldo)
        layout_ok(out)
        ref, scale, ref32 = cpu_step_edges.posterior64(y, ym, eps, zero, z, t, alphas, omabs)
        got = torch.from_numpy(out[:, :C].copy())
        # 35 operations on sum |terms| (posterior64's scale) + 4 |ref_cpu fp32 - float64|
        cpu_step_edges.assert_stage(got, ref, scale, f"listing UPDATE t={t}", tol=N_OPS_POSTERIOR * U, fp32_ref=ref32)
        # the oracle's fp32 path performs the same operations in the same order; torch's CPU kernels are not correctly rounded on every
        # host, so this is a figure, not an assertion
        print(f"{shape} t={t}: {int((got.double() != ref32).sum())} of {got.numel()} elements differ from ref_cpu's fp32 bits")
    out = L.reverse_step_f32(L.RSTEP_LAST, n["y"], n["ymean"], n["eps"], None, 1.0, float(omabs[0]), 0.0, ldo)
    layout_ok(out)
    ref, scale, ref32 = cpu_step_edges.posterior64(y, ym, eps, zero, None, 0, alphas, omabs)
    got = torch.from_numpy(out[:, :C].copy())
    # 10 operations on sum |terms| + 4 |ref_cpu fp32 - float64|
    cpu_step_edges.assert_stage(got, ref, scale, "listing LAST", tol=N_OPS_LAST * U, fp32_ref=ref32)


def plan_rows(omabs):
    """(name, (cy, cm, ce, cz)) of the three coefficient rows the GPU test uses: a mid-chain step at eta = 0 and at eta = 1, and row 0."""
    from nested_diffusion_amd.diffusion_utils import sampler_plan, timestep_sequence
    tau = timestep_sequence(T, 10)
    p0, p1 = sampler_plan(omabs, tau, 0.0), sampler_plan(omabs, tau, 1.0)
    assert float(p0.coef[5, 3]) == 0.0 and float(p1.coef[5, 3]) > 0.0 and float(p1.coef[0, 3]) == 0.0
    return [("eta0", tuple(float(v) for v in p0.coef[5])), ("eta1", tuple(float(v) for v in p1.coef[5])),
            ("row0", tuple(float(v) for v in p1.coef[0]))]


@needs_fmaf
@pytest.mark.parametrize("shape", SHAPES[1:5])
def test_reverse_step_coef_listing_against_float64(shape, tables):
    B, mc, C, ldo, ldy = shape
    io = step_inputs(B, mc, C, ldy, 200 * B + C)
    M = B * mc
    ym = io["ymean"][torch.arange(M) % B]
    n = {k: v.numpy() for k, v in io.items()}
    for name, (cy, cm, ce, cz) in plan_rows(tables[1]):
        out = L.reverse_step_coef_f32(n["y"], n["ymean"], n["eps"], n["z"], cy, cm, ce, cz, ldo)
        y, e, z = io["y"][:, :C].double(), io["eps"].double(), io["z"].double()
        ref = cy * y + cm * ym.double() + ce * e + cz * z
        mag = abs(cy) * y.abs() + abs(cm) * ym.double().abs() + abs(ce) * e.abs() + abs(cz) * z.abs()
        err = (torch.from_numpy(out[:, :C].copy()).double() - ref).abs()
        # 4 operations (the product and three fused multiply-adds) on sum |terms|
        assert bool((err <= 4 * U * mag).all()), (name, float((err / mag).max() / U))
        if ldo >= 2 * C:
            assert np.array_equal(out[:, C:2 * C], ym.numpy()) and not out[:, 2 * C:].any()
        if cz == 0.0:                                                                # z = NULL and cz = 0 with a draw: the same bits
            assert np.array_equal(out, L.reverse_step_coef_f32(n["y"], n["ymean"], n["eps"], None, cy, cm, ce, 0.0, ldo))


BWD_SHAPES = [(1, 1, 1, 1, None), (1, 1, 1, 2, 1), (3, 2, 2, 16, 16), (5, 3, 3, 6, 16), (5, 3, 3, 7, 4), (4, 2, 7, 64, 64), (33, 3, 8, 8, 9)]


@pytest.mark.parametrize("t", (0,) + TS)
def test_backward_coefficients_are_the_oracles_derivatives(t, tables):
    """ensemble_grad.reverse_step_coefficients row t against float64 autograd through the oracle's step: the step is affine, so the
    derivative of sum(out) with respect to each operand is the coefficient.  Formed in double, rounded once: U relative, and 1e-9 for
    the float64 cancellation of gamma_2 at t = 1 (5e-4 of headroom lost from 1e-16)."""
    from nested_diffusion_amd.ensemble_grad import reverse_step_coefficients
    alphas, omabs = tables
    coef = reverse_step_coefficients(alphas, omabs)[t].double()
    y, ym, eps = (torch.randn(4, 3, generator=gen(t + i), dtype=torch.float64).requires_grad_(True) for i in range(3))
    if t == 0:
        out = ref_cpu.p_sample_t_1to0_given_eps(y, ym, eps, omabs.double())
    else:
        out = ref_cpu.p_sample_given_eps(y, ym, eps, t, alphas.double(), omabs.double(), torch.zeros(4, 3, dtype=torch.float64))
    out.sum().backward()
    for c, g in zip(coef, (y.grad, ym.grad, eps.grad)):
        assert bool(((g - c).abs() <= U * c.abs() + 1e-9).all()), (t, float(c), float(g[0, 0]))


@pytest.mark.parametrize("want_deps", [True, False])
@pytest.mark.parametrize("shape", BWD_SHAPES)
def test_reverse_step_bwd_listing_against_float64_autograd(shape, want_deps, tables):
    """L = sum(step(y, ymean[r % B], eps) * g[:, :C]) + sum(ymean[r % B] * g[:, C:2C]) (the yhat half, ldg >= 2C) by float64 autograd
    through the oracle, with the fp32 coefficients of reverse_step_coefficients in the listing."""
    from nested_diffusion_amd.ensemble_grad import reverse_step_coefficients
    B, mc, C, ldg, lda = shape
    alphas, omabs = tables
    M = B * mc
    for t in (0, 1, 500):
        cy, cm, ce = (float(v) for v in reverse_step_coefficients(alphas, omabs)[t])
        gg = gen(1000 * t + 10 * B + C)
        g, before = torch.randn(M, ldg, generator=gg), torch.randn(B, C, generator=gg)
        y, eps = (torch.randn(M, C, generator=gg, dtype=torch.float64).requires_grad_(True) for _ in range(2))
        ym = torch.randn(B, C, generator=gg, dtype=torch.float64).requires_grad_(True)
        ymr = ym.repeat(mc, 1)
        if t == 0:
            out = ref_cpu.p_sample_t_1to0_given_eps(y, ymr, eps, omabs.double())
        else:
            out = ref_cpu.p_sample_given_eps(y, ymr, eps, t, alphas.double(), omabs.double(), torch.zeros(M, C, dtype=torch.float64))
        loss = (out * g[:, :C].double()).sum()
        if ldg >= 2 * C:
            loss = loss + (ymr * g[:, C:2 * C].double()).sum()
        loss.backward()
        deps, dyadd, dymean = L.reverse_step_bwd_f32(g.numpy(), C, cy, cm, ce, before.numpy(), lda, want_deps)
        assert (deps is None) == (not want_deps) and (dyadd is None) == (lda is None)
        slack = 1e-9 * g[:, :C].double().abs()                 # the float64 reference's own cancellation at small t (see above)
        if want_deps:                                          # 2 operations: the coefficient's rounding and the product
            assert bool(((torch.from_numpy(deps).double() - eps.grad).abs() <= 2 * U * eps.grad.abs() + slack).all())
        if lda is not None:                                    # 2 operations, and the padding columns are +0
            assert dyadd.shape == (M, lda) and not dyadd[:, C:].any() and not np.signbit(dyadd[:, C:]).any()
            assert bool(((torch.from_numpy(dyadd[:, :C].copy()).double() - y.grad).abs() <= 2 * U * y.grad.abs() + slack).all())
        terms = abs(cm) * g[:, :C].double().abs()
        if ldg >= 2 * C:
            terms = terms + g[:, C:2 * C].double().abs()
        mag = terms.reshape(mc, B, C).sum(0) + before.double().abs()
        n_ops = 3 * mc + 2       # per trial: the product, its addition, the yhat half's addition; the final addition; cm's own rounding
        err = (torch.from_numpy(dymean).double() - (before.double() + ym.grad)).abs()
        assert bool((err <= n_ops * U * mag + 1e-9 * mag).all()), (t, float((err / mag).max() / U), n_ops)


# ---- softmax, the block backward, the block product ----------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,C", [(1, 1), (1, 2), (127, 3), (129, 17), (3, 1000), (1000, 3)])
def test_softmax_bwd_listing_against_float64_autograd(rows, C):
    g = gen(rows + C)
    logits, dp = torch.randn(rows, C, generator=g) * 2, torch.randn(rows, C, generator=g)
    l64 = logits.double().requires_grad_(True)
    p64 = torch.softmax(l64, dim=1)
    (p64 * dp.double()).sum().backward()
    p = p64.detach().float()
    got = torch.from_numpy(L.softmax_bwd_f32(p.numpy(), dp.numpy())).double()
    mag = p.double() * (dp.double().abs() + (dp.double().abs() * p.double()).sum(1, keepdim=True))
    # 2C operations of the dot, the subtraction, the product, and p's own rounding to fp32 in the factor and in the dot
    n_ops = 2 * C + 4
    err = (got - l64.grad).abs()
    assert bool((err <= n_ops * U * mag).all()), float((err / mag).max() / U)
    if C == 1:
        assert not got.numpy().any() and not np.signbit(got.numpy()).any()         # p = 1: dp - dp * 1 = +0


@pytest.mark.parametrize("B,mc,N", [(1, 1, 1), (3, 2, 257), (5, 3, 16)])
def test_cond_act_bwd_listing_against_float64_autograd(B, mc, N):
    """The block out = softplus(a_t u + c) * mul[r % B] by float64 autograd: dL/du and dL/dmul for L = sum(out * dh)."""
    g = gen(7 * B + N)
    M = B * mc
    z = torch.rand(M, N, generator=g) * 80 - 40                                      # the pre-activation: both sides of the threshold 20
    for i, v in enumerate((-30.0, 16.0, -16.0, 20.0, 20.000002, 19.999998, 40.0, -40.0)):
        z.view(-1)[(7 * i) % z.numel()] = v
    h = torch.nn.functional.softplus(z.double()).float()                             # the taped output, rounded once
    dh, a = torch.randn(M, N, generator=g), torch.rand(N, generator=g) + 0.5
    mul, prev = torch.randn(B, N, generator=g), torch.randn(B, N, generator=g)
    u =((z.double() - 0.25) / a.double()).requires_grad_(True)                      # z = a_t u + c with c = 0.25
    m64 = mul.double().requires_grad_(True)
    out = torch.nn.functional.softplus(a.double() * u + 0.25, threshold=1e9) * m64.repeat(mc, 1)
    (out * dh.double()).sum().backward()
    du, exact, acc = L.cond_act_bwd_f32(dh.numpy(), h.numpy(), a.numpy(), mul.numpy(), prev.numpy(), B)
    assert np.array_equal(exact, (h > 20).numpy())
    if exact.any():
        # 2 operations (g = dh mul, g a_t; g * 1 is exact) and sigma(z) = 1 - 2e-9 at h > 20 taken as 1: under one more
        e = torch.from_numpy(exact)
        err = (torch.from_numpy(du).double() - u.grad)[e].abs()
        assert bool((err <= 3 * U * u.grad[e].abs()).all()) and bool(np.isnan(du[~exact]).all())
    else:
        assert du is None
    terms = (dh.double() * h.double()).reshape(mc, B, N)
    mag = terms.abs().sum(0) + prev.double().abs()
    # per trial the product and its addition, the final addition, and h's rounding to fp32: 2 mc + 2 <= the (mc + 2) of the GPU test + mc
    err = (torch.from_numpy(acc).double() - (prev.double() + m64.grad)).abs()
    assert bool((err <= (2 * mc + 2) * U * mag).all())
    # h None: no activation, every element exact, one or two operations
    du, exact, acc = L.cond_act_bwd_f32(dh.numpy(), None, a.numpy(), None, None, B)
    assert exact.all() and acc is None
    ref = dh.double() * a.double()
    assert bool(((torch.from_numpy(du).double() - ref).abs() <= U * ref.abs()).all())
    # the block product: one operation
    y = torch.from_numpy(L.cond_mul_f32(h.numpy(), mul.numpy())).double()
    ref = h.double() * mul.double().repeat(mc, 1)
    assert bool(((y - ref).abs() <= U * ref.abs()).all())
