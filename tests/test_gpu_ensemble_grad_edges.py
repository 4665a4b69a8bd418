"""Edge shapes and launch geometry of the ensemble-gradient kernels (csrc/nd_ensemble_grad.hip), each called ALONE through the C ABI:
leading dimensions and class counts the chain never uses (tests/test_gpu_ensemble_grad.py runs C in {2, 3}, every leading dimension 16,
one workgroup per launch), a second and a partial last workgroup of every kernel, the documented maxima, du == dh in place, a captured
line of all seven entry points, and the refusals.

Every output lies in the middle of a buffer of 0xFF bytes (a NaN in every fp32 element) with GUARD elements on each side, and so does every
input: an element left unwritten, or a read past an input, is a NaN in the result; after each call the guard bytes are compared.  Every
call runs twice into fresh buffers and the two results are equal bit for bit.  Inputs come from seeded CPU generators.

Rules of comparison, and the largest figure measured on the MI355X against each bound:
- nd_reverse_step INIT, the layout columns, nd_reverse_step_coef, nd_reverse_step_bwd, nd_softmax_bwd, nd_cond_mul, the dmul_acc of
  nd_cond_act_bwd and its du where the listing has no library function (h NULL, h > 20): BIT-EQUAL to the float32 restatement of the
  header's listings (tests/_ensemble_grad_listing.py, shown within its counted bounds of float64 by
  tests/test_ensemble_grad_listing_host.py).  Zero columns are +0.  Measured: 0 differing bits in every case.
- nd_reverse_step UPDATE and LAST: bit-equal to the restatement as well (division and square root are correctly rounded: build.py's
  FLAGS carry no fast-math flag), and within assert_stage / posterior64 of tests/test_gpu_step_edges.py: per element
  |got - float64| <= 1e-5 * sum |terms| + 4 |ref_cpu fp32 - float64|.  Measured: 0 ulp from the restatement; worst normalised error
  2.1e-7 against the bar 1e-5.
- du of nd_cond_act_bwd elsewhere: the 10 U rule of tests/test_gpu_ensemble_grad.py (three products and -expm1f at 3 ulp).
  Measured: 3.0 U.
- nd_aggregate_xent_bwd: relative L2 <= 1e-5 against float64 autograd (agg64 of tests/test_gpu_ensemble_grad.py), PER IMAGE for P, loss and
  dsamples[:, b].  Condition on the inputs, asserted: the same oracle in float32 autograd is within E32_MAX = 2.5e-6 of float64 per
  image (4 E32_MAX is the bar, the e32 rule of tests/test_gpu_ensemble_grad.py).  P is nd_aggregate's bit for bit.  Measured per
  image: P 2.6e-7, loss 4.4e-7, dsamples 2.9e-7.
Condition on the inputs of every bit comparison, asserted: finite, and no non-zero magnitude under 2^-40, so that no product with a schedule
coefficient comes near the subnormal range."""
import math

import numpy as np
import pytest
import torch

import _ensemble_grad_listing as L
from oracle import ref_cpu
from test_gpu_ensemble_grad import TAU, U, act_ref64, agg64
from test_gpu_grad_edges import check, lib, p, poisoned, stream
from test_gpu_step_edges import assert_stage, posterior64

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 256                          # fp32 elements of 0xFF bytes on each side of an output
E32_MAX = 2.5e-6
T_SCHED = 1000
needs_fmaf = pytest.mark.skipif(not L.HAVE_FMAF, reason=L.FMAF_MISSING)
FIGURES = {}                         # name -> the largest figure of this module's run, printed at its end


def gen(seed):
    return torch.Generator().manual_seed(seed)


def note(name, value):
    FIGURES[name] = max(FIGURES.get(name, 0.0), float(value))


@pytest.fixture(scope="module", autouse=True)
def report_figures():
    yield
    for name, v in sorted(FIGURES.items()):
        print(f"\nlargest {name}: {v:.3e}", end="")


class Guarded:
    """An fp32 tensor of `shape` in the middle of a 0xFF buffer; init: what it holds before the call (an in-place operand, an input)."""

    def __init__(self, *shape, init=None):
        self.n = math.prod(shape)
        self.buf = poisoned(self.n + 2 * GUARD)
        self.t = self.buf[GUARD:GUARD + self.n].view(*shape)
        if init is not None:
            self.t.copy_(init.reshape(shape))

    def result(self, what):
        """The tensor on the host, after: every element written (no NaN), the guards untouched."""
        torch.cuda.synchronize()
        raw = self.buf.view(torch.int32)
        assert bool((raw[:GUARD] == -1).all()), f"{what}: bytes before the output changed"
        assert bool((raw[GUARD + self.n:] == -1).all()), f"{what}: bytes after the output changed"
        out = self.t.cpu()
        assert not bool(out.isnan().any()), f"{what}: {int(out.isnan().sum())} elements unwritten or NaN"
        return out


def dev_in(t):
    """An input on the device with NaNs on both sides of it."""
    return None if t is None else Guarded(*t.shape, init=t).t


def twice(fn):
    a, b = fn(), fn()
    for x, y in zip(a, b):
        assert (x is None and y is None) or torch.equal(x, y), "two runs differ"
    return a


def usable(*tensors):
    """The condition on the inputs of a bit comparison."""
    for t in tensors:
        if t is not None:
            a = torch.as_tensor(t).abs()
            assert bool(a.isfinite().all()) and not bool(((a > 0) & (a < 2.0 ** -40)).any()), "a bad draw: the test's inputs, not the kernel"


def ulps(got, want):
    """Largest distance in units of the last place between two float32 arrays of one sign pattern (0 when bit-equal)."""
    a, b = np.ascontiguousarray(got, np.float32).view(np.int32).astype(np.int64), np.ascontiguousarray(want, np.float32).view(np.int32).astype(np.int64)
    a, b = np.where(a < 0, -(a & 0x7FFFFFFF), a), np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return int(np.abs(a - b).max()) if a.size else 0


def assert_bits(got, want, what):
    got, want = got.numpy() if isinstance(got, torch.Tensor) else got, np.asarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    same = got.view(np.int32) == want.view(np.int32)
    if not same.all():
        i = tuple(int(v) for v in np.argwhere(~same)[0])
        raise AssertionError(f"{what}: {int((~same).sum())} of {same.size} elements differ in bits, first at {i}: got {got[i]!r}, want {want[i]!r}; "
                             f"largest distance {ulps(got, want)} ulp")


@pytest.fixture(scope="module")
def tables():
    return ref_cpu.schedule_tables("linear", T_SCHED, 1e-4, 0.02)


# ---- 1. nd_reverse_step and nd_reverse_step_coef ---------------------------------------------------------------------------------------
# (B, mc, C, ldo, ldy)
RS_CASES = [(1, 1, 1, 1, 1),               # the smallest shape
            (1, 1, 1, 2, 64),              # ldo = 2C at C = 1
            (3, 2, 2, 16, 16),             # the chain's own
            (7, 1, 5, 10, 9),              # ldo == 2C: no zero column
            (5, 3, 3, 7, 5),               # one zero column, ldy != ldo
            (33, 2, 8, 64, 64),            # 4224 elements: the 17th workgroup is half full
            (128, 64, 8, 8, 8)]            # M = 8192, the documented maximum
RS_T = (1, 2, 500, 999)


def rs_inputs(B, mc, C, ldy, seed):
    g = gen(seed)
    M = B * mc
    io = dict(y=torch.randn(M, ldy, generator=g), ymean=torch.softmax(torch.randn(B, C, generator=g), -1),
              eps=torch.randn(M, C, generator=g), z=torch.randn(M, C, generator=g))
    usable(*io.values())
    return io, {k: dev_in(v) for k, v in io.items()}


def reverse_step_abi(mode, d, ldy, ldo, M, B, C, alpha_t, s_t, s_tm1):
    out = Guarded(M, ldo)
    check(lib().nd_reverse_step(mode, p(d["y"]) if mode != L.RSTEP_INIT else None, ldy, p(d["ymean"]), p(d["eps"]) if mode != L.RSTEP_INIT else None,
                                p(d["z"]) if mode != L.RSTEP_LAST else None, p(out.t), ldo, M, B, C, alpha_t, s_t, s_tm1, stream()),
          "nd_reverse_step")
    return (out.result(f"nd_reverse_step mode {mode}"),)


@pytest.mark.parametrize("case", RS_CASES, ids=lambda c: "B{}_mc{}_C{}_ldo{}_ldy{}".format(*c))
def test_reverse_step_alone(case, tables):
    B, mc, C, ldo, ldy = case
    alphas, omabs = tables
    M = B * mc
    io, d = rs_inputs(B, mc, C, ldy, 31 * B + 7 * C + ldo)
    n = {k: v.numpy() for k, v in io.items()}
    rows = torch.arange(M) % B
    ym_rows, zero = io["ymean"][rows].to(DEV), torch.zeros(M, C, dtype=torch.float64, device=DEV)
    got, = twice(lambda: reverse_step_abi(L.RSTEP_INIT, d, ldy, ldo, M, B, C, 1.0, 0.0, 0.0))
    assert_bits(got, L.reverse_step_f32(L.RSTEP_INIT, None, n["ymean"], None, n["z"], 1.0, 0.0, 0.0, ldo), "INIT")
    worst_ulp = 0
    for t in RS_T + (0,):
        mode = L.RSTEP_UPDATE if t else L.RSTEP_LAST
        a, s, s1 = (float(alphas[t]), float(omabs[t]), float(omabs[t - 1])) if t else (1.0, float(omabs[0]), 0.0)
        got, = twice(lambda: reverse_step_abi(mode, d, ldy, ldo, M, B, C, a, s, s1))
        want = L.reverse_step_f32(mode, n["y"], n["ymean"], n["eps"], n["z"] if t else None, a, s, s1, ldo)
        assert_bits(got[:, C:].contiguous(), want[:, C:], f"layout columns t={t}")
        ref, scale, ref32 = posterior64(d["y"][:, :C], ym_rows, d["eps"], zero, d["z"] if t else None, t, alphas, omabs)
        assert_stage(got[:, :C].to(DEV), ref, scale, f"edges {'UPDATE' if t else 'LAST'}: t={t} {case}", fp32_ref=ref32)
        err = ((got[:, :C].to(DEV).double() - ref).abs() - 4 * (ref32 - ref).abs()).clamp_min(0) / scale
        note("normalised error of UPDATE / LAST against float64 (bar 1e-5)", err.max())
        worst_ulp = max(worst_ulp, ulps(got[:, :C].numpy(), want[:, :C]))
        assert_bits(got[:, :C].contiguous(), np.ascontiguousarray(want[:, :C]), f"{'UPDATE' if t else 'LAST'} t={t}")
    note("ulp distance of UPDATE / LAST from the restatement", worst_ulp)
    print(f"reverse_step {case}: INIT, layout, UPDATE t={RS_T} and LAST bit-equal to the restatement")


def coefficient_rows(omabs):
    """A mid-chain step of a 10-step plan at eta = 0 (cz = 0) and at eta = 1, and the plan's row 0 (the last step, cz = 0)."""
    from nested_diffusion_amd.diffusion_utils import sampler_plan, timestep_sequence
    tau = timestep_sequence(T_SCHED, 10)
    p0, p1 = sampler_plan(omabs, tau, 0.0), sampler_plan(omabs, tau, 1.0)
    rows = {"eta0": p0.coef[5], "eta1": p1.coef[5], "row0": p1.coef[0]}
    assert float(rows["eta0"][3]) == 0.0 and float(rows["eta1"][3]) > 0.0 and float(rows["row0"][3]) == 0.0
    return {k: tuple(float(x) for x in v) for k, v in rows.items()}


def reverse_step_coef_abi(d, with_z, ldy, ldo, M, B, C, coef):
    out = Guarded(M, ldo)
    check(lib().nd_reverse_step_coef(p(d["y"]), ldy, p(d["ymean"]), p(d["eps"]), p(d["z"]) if with_z else None, p(out.t), ldo, M, B, C, *coef,
                                     stream()), "nd_reverse_step_coef")
    return (out.result("nd_reverse_step_coef"),)


@needs_fmaf
@pytest.mark.parametrize("case", RS_CASES, ids=lambda c: "B{}_mc{}_C{}_ldo{}_ldy{}".format(*c))
def test_reverse_step_coef_alone(case, tables):
    """The sampler's bits: fmaf(cz, z, fmaf(ce, eps, fmaf(cm, ymean, cy * y))) with the C library's fmaf."""
    B, mc, C, ldo, ldy = case
    M = B * mc
    io, d = rs_inputs(B, mc, C, ldy, 37 * B + 5 * C + ldo)
    n = {k: v.numpy() for k, v in io.items()}
    for name, coef in coefficient_rows(tables[1]).items():
        usable(torch.tensor(coef))
        want = L.reverse_step_coef_f32(n["y"], n["ymean"], n["eps"], n["z"], *coef, ldo)
        got, = twice(lambda: reverse_step_coef_abi(d, True, ldy, ldo, M, B, C, coef))
        assert_bits(got, want, f"coef {name}, z given")
        if coef[3] == 0.0:                                    # fmaf(0, z, v) = v for a finite z: the same bits without the draw
            got, = twice(lambda: reverse_step_coef_abi(d, False, ldy, ldo, M, B, C, coef))
            assert_bits(got, want, f"coef {name}, z = NULL")
    print(f"reverse_step_coef {case}: three coefficient rows bit-equal to the restatement")


# ---- 2. nd_reverse_step_bwd ---------------------------------------------------------------------------------------------------------------
# (B, mc, C, ldg, lda); lda None: no dyadd
BWD_CASES = [(1, 1, 1, 1, None),
             (1, 1, 1, 2, 1),              # the yhat half at C = 1
             (3, 2, 2, 16, 16),
             (5, 3, 3, 6, 16),             # ldg == 2C, and lda - C = 13 is not a multiple of 3
             (5, 3, 3, 7, 4),
             (4, 2, 7, 64, 64),
             (33, 3, 8, 8, 9),             # B * C = 264: a second workgroup with 8 live threads
             (128, 2, 8, 16, 64)]          # four full workgroups


def reverse_step_bwd_abi(g_dev, before, ldg, lda, want_deps, M, B, C, cy, cm, ce):
    deps = Guarded(M, C) if want_deps else None
    dyadd = Guarded(M, lda) if lda is not None else None
    dymean = Guarded(B, C, init=before)
    check(lib().nd_reverse_step_bwd(p(g_dev), ldg, cy, cm, ce, p(deps.t) if deps else None, p(dyadd.t) if dyadd else None,
                                    lda if lda is not None else 0, p(dymean.t), M, B, C, stream()), "nd_reverse_step_bwd")
    return (deps.result("deps") if deps else None, dyadd.result("dyadd") if dyadd else None, dymean.result("dymean"))


@pytest.mark.parametrize("want_deps", [True, False], ids=["deps", "no_deps"])
@pytest.mark.parametrize("case", BWD_CASES, ids=lambda c: "B{}_mc{}_C{}_ldg{}_lda{}".format(*c))
def test_reverse_step_bwd_alone(case, want_deps, tables):
    """g lies between NaNs: with ldg == C a thread that took columns C .. 2C-1 for a yhat half, or any read past the last row, makes
    dymean NaN.  dymean starts from non-zero values."""
    from nested_diffusion_amd.ensemble_grad import reverse_step_coefficients
    B, mc, C, ldg, lda = case
    M = B * mc
    gg = gen(41 * B + 3 * C + ldg)
    g, before = torch.randn(M, ldg, generator=gg), torch.randn(B, C, generator=gg) + 3.0
    usable(g, before)
    g_dev = dev_in(g)
    coefs = reverse_step_coefficients(*tables)
    for t in (1, 500):
        cy, cm, ce = (float(v) for v in coefs[t])
        usable(coefs[t])
        deps, dyadd, dymean = twice(lambda: reverse_step_bwd_abi(g_dev, before, ldg, lda, want_deps, M, B, C, cy, cm, ce))
        w_deps, w_dyadd, w_dymean = L.reverse_step_bwd_f32(g.numpy(), C, cy, cm, ce, before.numpy(), lda, want_deps)
        assert bool(dymean.isfinite().all())
        assert_bits(dymean, w_dymean, f"dymean t={t}")
        if want_deps:
            assert_bits(deps, w_deps, f"deps t={t}")
        if lda is not None:
            assert_bits(dyadd, w_dyadd, f"dyadd t={t} (columns C .. lda-1 are +0)")
    print(f"reverse_step_bwd {case} deps={want_deps}: bit-equal to the restatement")


# ---- 3. nd_aggregate_xent_bwd -------------------------------------------------------------------------------------------------------------
# (B, C, S, tau): every B of {1, 64, 65, 130}, every C of {1, 2, 8, 15, 16}, every S of {1, 2, 37}, both temperatures
AGG_CASES = [(1, 1, 1, TAU), (1, 2, 2, 1.0), (1, 16, 37, TAU), (1, 8, 1, 1.0),
             (64, 1, 2, 1.0), (64, 2, 37, TAU), (64, 8, 1, TAU), (64, 15, 2, 1.0), (64, 16, 1, TAU),
             (65, 1, 37, TAU), (65, 2, 1, 1.0), (65, 8, 2, TAU), (65, 15, 37, 1.0), (65, 16, 2, TAU),
             (130, 1, 1, 1.0), (130, 2, 2, TAU), (130, 8, 37, 1.0), (130, 15, 1, TAU), (130, 16, 37, TAU), (130, 16, 37, 1.0)]


def agg32(samples, labels, tau):
    """agg64's computation in float32 autograd: the condition on the inputs."""
    y = samples.clone().requires_grad_(True)
    P = ref_cpu.compute_ensemble_confidence(list(y.unbind(0)), tau)
    loss = -torch.log(P[torch.arange(P.shape[0]), labels])
    loss.sum().backward()
    return P.detach(), loss.detach(), y.grad


def per_image_rel_l2(got, want):
    """||got_b - want_b|| / ||want_b|| for every image b: P [B, C], loss [B], dsamples [S, B, C]."""
    got, want = got.double().cpu(), want.double().cpu()
    if got.dim() == 3:
        got, want = got.transpose(0, 1), want.transpose(0, 1)
    got, want = got.reshape(got.shape[0], -1), want.reshape(want.shape[0], -1)
    return (got - want).norm(dim=1) / want.norm(dim=1)


def aggregate_abi(samples_dev, labels_dev, S, B, C, tau):
    P, loss, ds = Guarded(B, C), Guarded(B), Guarded(S, B, C)
    check(lib().nd_aggregate_xent_bwd(p(samples_dev), p(labels_dev), p(P.t), p(loss.t), p(ds.t), S, B, C, tau, stream()), "nd_aggregate_xent_bwd")
    return P.result("P"), loss.result("loss"), ds.result("dsamples")


@pytest.mark.parametrize("case", AGG_CASES, ids=lambda c: "B{}_C{}_S{}_tau{}".format(*c))
def test_aggregate_xent_alone(case):
    from nested_diffusion_amd import ops
    B, C, S, tau = case
    g = gen(1000 * B + 10 * C + S)
    samples = torch.randn(S, B, C, generator=g) * 0.2 + 0.5
    labels = torch.randint(0, C, (B,), generator=g)
    sd, ld = dev_in(samples), labels.to(DEV)
    P, loss, ds = twice(lambda: aggregate_abi(sd, ld, S, B, C, tau))
    assert torch.equal(P, ops.aggregate(samples.to(DEV), tau)[0].cpu()), "P does not carry nd_aggregate's bits"
    if C == 1:
        assert bool((P == 1).all()) and bool((loss == 0).all()) and bool((ds == 0).all())
        return
    ref, r32 = agg64(samples, labels, tau), agg32(samples, labels, tau)
    for name, got, want, w32 in zip(("P", "loss", "dsamples"), (P, loss, ds), ref, r32):
        e32, r = per_image_rel_l2(w32, want), per_image_rel_l2(got, want)
        print(f"aggregate {case} {name}: per image e32 <= {float(e32.max()):.3e}, gpu <= {float(r.max()):.3e}")
        note(f"per-image rel-L2 of the aggregation's {name} (bar 1e-5)", r.max())
        assert float(e32.max()) <= E32_MAX, (name, "the inputs are ill-conditioned", float(e32.max()))
        assert bool((r <= 1e-5).all()), (name, case, "images", (r > 1e-5).nonzero().flatten()[:8].tolist(), float(r.max()))


@pytest.mark.parametrize("b", [63, 64, 129])
def test_aggregate_conventions_in_a_later_workgroup(b):
    """The conventions of test_aggregate_xent_grad_conventions_and_refusals at image b of B = 130: only that image's outputs change."""
    from nested_diffusion_amd import ops
    S, B, C = 4, 130, 3
    g = gen(300 + b)
    samples = torch.randn(S, B, C, generator=g) * 0.5 + 0.5
    labels = torch.randint(0, C, (B,), generator=g)
    y = int(labels[b])
    clean = [t.cpu() for t in ops.aggregate_xent_grad(samples.to(DEV), TAU, labels.to(DEV))]
    assert all(bool(t.isfinite().all()) for t in clean)
    others = torch.arange(B) != b

    def rest_unchanged(got):
        return (torch.equal(got[0][others], clean[0][others]) and torch.equal(got[1][others], clean[1][others])
                and torch.equal(got[2][:, others], clean[2][:, others]))

    under = samples.clone()
    under[:, b, y] = 13.0                                      # -(12^2) / 0.2555 is 560 below the row's largest logit
    got = [t.cpu() for t in ops.aggregate_xent_grad(under.to(DEV), TAU, labels.to(DEV))]
    assert float(got[1][b]) == float("inf") and bool((got[2][:, b] == 0).all()) and float(got[0][b, y]) == 0.0 and rest_unchanged(got)
    nan = samples.clone()
    nan[2, b, 0] = float("nan")
    got = [t.cpu() for t in ops.aggregate_xent_grad(nan.to(DEV), TAU, labels.to(DEV))]
    assert bool(got[0][b].isnan().all()) and bool(got[1][b].isnan()) and bool(got[2][:, b].isnan().all()) and rest_unchanged(got)
    for wrong in (C, -1):
        bad = labels.clone()
        bad[b] = wrong
        with pytest.raises(ValueError, match="labels"):
            ops.aggregate_xent_grad(samples.to(DEV), TAU, bad.to(DEV))
        got = [t.cpu() for t in ops.aggregate_xent_grad(samples.to(DEV), TAU, bad.to(DEV), check_labels=False)]
        assert bool(got[1][b].isnan()) and bool((got[2][:, b] == 0).all()) and torch.equal(got[0], clean[0]) and rest_unchanged(got)


# ---- 4. nd_softmax_bwd ----------------------------------------------------------------------------------------------------------------------
SOFTMAX_CASES = [(rows, C) for rows in (1, 127, 128, 129, 1000) for C in (1, 2, 3, 17)] + [(1, 1000), (3, 1000)]


@pytest.mark.parametrize("rows,C", SOFTMAX_CASES)
def test_softmax_bwd_alone(rows, C):
    g = gen(rows + 3 * C)
    prob, dp = torch.softmax(torch.randn(rows, C, generator=g) * 2, dim=1), torch.randn(rows, C, generator=g)
    usable(prob, dp)
    pd, dd = dev_in(prob), dev_in(dp)

    def run():
        out = Guarded(rows, C)
        check(lib().nd_softmax_bwd(p(pd), p(dd), p(out.t), rows, C, stream()), "nd_softmax_bwd")
        return (out.result("dlogits"),)
    got, = twice(run)
    assert_bits(got, L.softmax_bwd_f32(prob.numpy(), dp.numpy()), f"softmax_bwd rows={rows} C={C}")
    if C == 1:
        assert bool((prob == 1).all()) and not bool(got.numpy().view(np.int32).any())          # +0 everywhere


# ---- 5. nd_cond_mul and nd_cond_act_bwd -------------------------------------------------------------------------------------------------
def act_inputs(B, mc, N, seed):
    """As act_inputs of tests/test_gpu_ensemble_grad.py (z spans [-40, 40] and takes the threshold 20 and its neighbours), and a_t,
    mul, the dmul_acc before the call: non-zero."""
    g = gen(seed)
    M = B * mc
    z = torch.rand(M, N, generator=g) * 80 - 40
    for i, v in enumerate((-30.0, 16.0, -16.0, 20.0, 20.000002, 19.999998, 40.0, -40.0)):
        z.view(-1)[(7 * i) % z.numel()] = v
    h = torch.nn.functional.softplus(z.double()).float()
    io = dict(dh=torch.randn(M, N, generator=g), h=h, a=torch.rand(N, generator=g) + 0.5, mul=torch.randn(B, N, generator=g),
              prev=torch.randn(B, N, generator=g) + 3.0)
    usable(io["dh"], io["a"], io["mul"], io["prev"])
    return io


def cond_act_abi(io, B, with_h, with_mul, in_place):
    M, N = io["dh"].shape
    dh = Guarded(M, N, init=io["dh"])
    du = dh if in_place else Guarded(M, N)
    acc = Guarded(B, N, init=io["prev"]) if with_mul else None
    h, a, mul = dev_in(io["h"]) if with_h else None, dev_in(io["a"]), dev_in(io["mul"]) if with_mul else None
    check(lib().nd_cond_act_bwd(p(dh.t), p(h), p(a), p(mul), p(du.t), p(acc.t) if acc else None, M, N, B, stream()), "nd_cond_act_bwd")
    return du.result("du"), acc.result("dmul_acc") if acc else None


@pytest.mark.parametrize("B,mc,N", [(3, 2, 255), (3, 2, 256), (3, 2, 257), (65535, 1, 1)])
def test_cond_mul_and_cond_act_bwd_alone(B, mc, N):
    """N one short of, at and one past a 256-column block; B at the grid-y limit.  du == dh in place equals the out-of-place result."""
    io = act_inputs(B, mc, N, 13 * N + mc)
    M = B * mc
    n = {k: v.numpy() for k, v in io.items()}
    sd, md = dev_in(io["h"]), dev_in(io["mul"])

    def mul_run():
        y = Guarded(M, N)
        check(lib().nd_cond_mul(p(sd), p(md), p(y.t), M, N, B, stream()), "nd_cond_mul")
        return (y.result("cond_mul"),)
    y, = twice(mul_run)
    assert_bits(y, L.cond_mul_f32(n["h"], n["mul"]), "cond_mul")
    for with_h, with_mul in ((True, True), (True, False), (False, False)):
        du, acc = twice(lambda: cond_act_abi(io, B, with_h, with_mul, False))
        du_in, acc_in = twice(lambda: cond_act_abi(io, B, with_h, with_mul, True))
        assert torch.equal(du_in, du) and (acc is None or torch.equal(acc_in, acc)), "du == dh in place differs from the out-of-place call"
        w_du, exact, w_acc = L.cond_act_bwd_f32(n["dh"], n["h"] if with_h else None, n["a"], n["mul"] if with_mul else None,
                                                n["prev"] if with_mul else None, B)
        if with_mul:
            assert_bits(acc, w_acc, "dmul_acc")
        if w_du is not None:
            assert_bits(du.numpy()[exact], w_du[exact], f"du where the listing is exact (h={with_h}, mul={with_mul})")
        want, _, _ = act_ref64(io["dh"], io["h"] if with_h else None, io["a"], io["mul"] if with_mul else None, io["prev"] if with_mul else None, B)
        err = (du.double() - want).abs() / want.abs().clamp_min(1e-38)
        note("error of du in U (bar 10)", err.max() / U)
        assert bool(((du.double() - want).abs() <= 10 * U * want.abs() + 1e-38).all()), (with_h, with_mul)


def test_cond_kernels_refuse_65536_images():
    t = torch.ones(65536, 1, device=DEV)
    out = torch.full((65536, 1), 7.0, device=DEV)
    assert lib().nd_cond_mul(p(t), p(t), p(out), 65536, 1, 65536, None) != 0
    assert lib().nd_cond_act_bwd(p(t), p(t), p(t[0]), None, p(out), None, 65536, 1, 65536, None) != 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---- 6. capture -------------------------------------------------------------------------------------------------------------------------------
def test_a_captured_line_of_all_entry_points_replays_the_eager_bits(tables):
    """INIT -> coef -> cond_mul -> cond_act_bwd -> reverse_step_bwd -> aggregate_xent_bwd -> softmax_bwd on one stream, each launch reading
    what the one before wrote; pre-allocated buffers, the raw ABI.  Two replays, the in-place operands restored before each."""
    B, mc, C, LD = 3, 2, 2, 16
    M = B * mc
    g = gen(77)
    z0, z1, eps = (torch.randn(M, C, generator=g).to(DEV) for _ in range(3))
    ymean = torch.softmax(torch.randn(B, C, generator=g), -1).to(DEV)
    mul, a_t = torch.randn(B, LD, generator=g).to(DEV), (torch.rand(LD, generator=g) + 0.5).to(DEV)
    h = torch.nn.functional.softplus(torch.randn(M, LD, generator=g) * 8).to(DEV)
    acc0, dymean0 = torch.randn(B, LD, generator=g).to(DEV), torch.randn(B, C, generator=g).to(DEV)
    labels = torch.tensor([0, 1, 1], device=DEV)
    coef = coefficient_rows(tables[1])["eta1"]
    new = lambda *s: poisoned(*s)                              # noqa: E731
    buf = dict(yT=new(M, LD), y1=new(M, LD), y2=new(M, LD), du=new(M, LD), deps=new(M, C), dyadd=new(M, LD), P=new(B, C), loss=new(B),
               ds=new(mc, B, C), dlogits=new(B, C), acc=acc0.clone(), dymean=dymean0.clone())
    nd = lib()

    def line():
        s = stream()
        check(nd.nd_reverse_step(L.RSTEP_INIT, None, C, p(ymean), None, p(z0), p(buf["yT"]), LD, M, B, C, 1.0, 0.0, 0.0, s), "INIT")
        check(nd.nd_reverse_step_coef(p(buf["yT"]), LD, p(ymean), p(eps), p(z1), p(buf["y1"]), LD, M, B, C, *coef, s), "coef")
        check(nd.nd_cond_mul(p(buf["y1"]), p(mul), p(buf["y2"]), M, LD, B, s), "cond_mul")
        check(nd.nd_cond_act_bwd(p(buf["y2"]), p(h), p(a_t), p(mul), p(buf["du"]), p(buf["acc"]), M, LD, B, s), "cond_act_bwd")
        check(nd.nd_reverse_step_bwd(p(buf["du"]), LD, 0.75, -0.5, 1.25, p(buf["deps"]), p(buf["dyadd"]), LD, p(buf["dymean"]), M, B, C, s), "bwd")
        check(nd.nd_aggregate_xent_bwd(p(buf["deps"]), p(labels), p(buf["P"]), p(buf["loss"]), p(buf["ds"]), mc, B, C, TAU, s), "aggregate")
        check(nd.nd_softmax_bwd(p(buf["P"]), p(buf["ds"]), p(buf["dlogits"]), B, C, s), "softmax_bwd")

    def restore(poison):
        for k, v in buf.items():
            if k == "acc":
                v.copy_(acc0)
            elif k == "dymean":
                v.copy_(dymean0)
            elif poison:
                v.view(torch.int32).fill_(-1)

    line()
    torch.cuda.synchronize()
    eager = {k: v.clone() for k, v in buf.items()}
    assert not any(bool(v.isnan().any()) for v in eager.values())              # every output written (torch.equal needs no NaN)
    assert not torch.equal(eager["acc"], acc0) and not torch.equal(eager["dymean"], dymean0)
    restore(True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        line()
    for _ in range(2):
        restore(True)
        graph.replay()
        torch.cuda.synchronize()
        for k, v in buf.items():
            assert torch.equal(v, eager[k]), f"replay differs from eager in {k}"


# ---- 7. refusals, each before any launch --------------------------------------------------------------------------------------------------
def test_refusals_leave_the_output_untouched():
    nd = lib()
    n = 8193 * 65                                              # every shape below fits: a refusal that were missing would stay in bounds
    z, out = torch.zeros(n, device=DEV), torch.full((n,), 7.0, device=DEV)
    zz, oo = p(z), p(out)
    other = torch.zeros(n, device=DEV)
    C = 4
    ok = dict(ldy=4, ldo=4, M=6, B=3, C=C)

    def step(mode=1, **kw):
        a = dict(ok, **kw)
        return nd.nd_reverse_step(mode, zz, a["ldy"], zz, zz, zz, oo, a["ldo"], a["M"], a["B"], a["C"], 1.0, 0.5, 0.5, None)

    def coef(cy=1.0, cm=0.5, ce=0.25, cz=0.0, z_ptr=zz, **kw):
        a = dict(ok, **kw)
        return nd.nd_reverse_step_coef(zz, a["ldy"], zz, zz, z_ptr, oo, a["ldo"], a["M"], a["B"], a["C"], cy, cm, ce, cz, None)

    def bwd(lda=4, dyadd=oo, **kw):
        a = dict(ok, **kw)
        return nd.nd_reverse_step_bwd(zz, a["ldo"], 1.0, 1.0, 1.0, None, dyadd, lda, p(other), a["M"], a["B"], a["C"], None)

    for mode in (1, 2):
        assert step(mode, ldy=C - 1) != 0 and step(mode, ldy=65) != 0
    for mode in (0, 1, 2):
        assert step(mode, ldo=65) != 0 and step(mode, M=8193, B=1) != 0 and step(mode, C=0, ldo=0, ldy=0) != 0 and step(mode, C=0) != 0
    assert coef(ldy=C - 1) != 0 and coef(ldy=65) != 0 and coef(ldo=65) != 0 and coef(M=8193, B=1) != 0 and coef(C=0) != 0
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert coef(cy=bad) != 0 and coef(cm=bad) != 0 and coef(ce=bad) != 0 and coef(cz=bad) != 0
    assert coef(cz=0.5, z_ptr=None) != 0                       # a draw's coefficient without the draw
    assert bwd(lda=C - 1) != 0 and bwd(lda=65) != 0 and bwd(M=8193, B=1) != 0 and bwd(C=0) != 0 and bwd(ldo=65) != 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((other == 0).all())
    assert coef(z_ptr=None) == 0 and step(1) == 0 and bwd() == 0                 # the accepted calls next to them are accepted
    torch.cuda.synchronize()
