"""Sampler plans (strided timesteps, generalized eta update) on the host: the timestep sequences, the coefficients against an independent
float64 restatement of the formulas of include/nested_diffusion.h ("SAMPLER PLAN"), the eta = 1 plan against the reference's own posterior
arithmetic on the derived tables (oracle/ref_cpu.py), the CLI surface and its refusals, nd_set_sampler's argument checks (refused before
any HIP call: no GPU here) and the exported symbols.  The GPU side: test_gpu_strided_sampler.py."""
import argparse
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from oracle import ref_cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"nd_set_sampler": 5, "nd_sampler_steps": 1, "nd_reverse_step_coef": 15}


# ---- sequences ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skip_type", ["uniform", "quadratic"])
@pytest.mark.parametrize("T,S", [(20, 5), (50, 10), (1000, 20), (1000, 100), (1000, 999), (7, 2), (2, 2), (1000, 500), (3, 2)])
def test_timestep_sequence_starts_at_0_ends_at_the_last_timestep_and_increases(T, S, skip_type):
    from nested_diffusion_amd.diffusion_utils import timestep_sequence
    tau = timestep_sequence(T, S, skip_type)
    assert tau[0] == 0 and tau[-1] == T - 1 and 2 <= len(tau) <= S
    assert all(isinstance(t, int) for t in tau) and all(b > a for a, b in zip(tau, tau[1:]))
    # the documented rule, restated with numpy in double: rounded, de-duplicated
    pts = np.linspace(0.0, T - 1.0, S) if skip_type == "uniform" else np.linspace(0.0, math.sqrt(T - 1.0), S) ** 2
    want = sorted(set(int(v) for v in np.round(pts)) | {0, T - 1})
    assert tau == want


def test_timestep_sequence_edges_and_refusals():
    from nested_diffusion_amd.diffusion_utils import timestep_sequence
    for skip_type in ("uniform", "quadratic"):
        assert timestep_sequence(1000, 1, skip_type) == [0] and timestep_sequence(1, 1, skip_type) == [0]
        assert timestep_sequence(9, 9, skip_type) == list(range(9)) and timestep_sequence(9, 4000, skip_type) == list(range(9))
    assert timestep_sequence(1000, 20) == [round(999 * i / 19) for i in range(20)]
    assert len(timestep_sequence(20, 15, "quadratic")) < 15                    # duplicates near 0 are dropped: S may shrink
    with pytest.raises(ValueError, match="S=0"):
        timestep_sequence(10, 0)
    with pytest.raises(ValueError, match="S=-3"):
        timestep_sequence(10, -3)
    with pytest.raises(ValueError, match="skip_type"):
        timestep_sequence(10, 5, "cosine")
    with pytest.raises(ValueError, match="T=0"):
        timestep_sequence(0, 1)


# ---- coefficients ------------------------------------------------------------------------------------------------------------------------
def coef64(omabs, tau, eta):
    """[S][4] (cy, cm, ce, cz) in python floats (double) from the fp32 table, straight from the issue's formulas."""
    s = [float(v) for v in omabs.tolist()]
    ab = [1.0 - s[t] * s[t] for t in tau]
    a = ab[0]
    rows = [[1 / math.sqrt(a), -(1 - math.sqrt(a)) / math.sqrt(a), -math.sqrt(1 - a) / math.sqrt(a), 0.0]]
    for j in range(1, len(tau)):
        at, ar = ab[j], ab[j - 1]
        sigma = eta * math.sqrt((1 - ar) / (1 - at)) * math.sqrt(1 - at / ar)
        cy = math.sqrt(ar / at)
        rows.append([cy, 1 - cy, math.sqrt(max(1 - ar - sigma * sigma, 0.0)) - cy * math.sqrt(1 - at), sigma])
    return rows


@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("T,tau", [(20, [2, 3, 9, 17]), (20, [0]), (20, [19]), (20, [0, 19]), (20, list(range(20))), (1000, None), (1000, "quadratic")])
def test_sampler_plan_matches_the_float64_formulas(T, tau, eta):
    from nested_diffusion_amd.diffusion_utils import sampler_plan, timestep_sequence
    _, omabs = ref_cpu.schedule_tables("linear", T, 1e-4, 0.02)
    if tau is None or tau == "quadratic":
        tau = timestep_sequence(T, 20, "uniform" if tau is None else "quadratic")
    ts, coef = sampler_plan(omabs, tau, eta)
    assert ts.dtype == torch.int32 and ts.tolist() == tau
    assert coef.dtype == torch.float32 and tuple(coef.shape) == (len(tau), 4) and coef.is_contiguous()
    want = torch.tensor(coef64(omabs, tau, eta), dtype=torch.float64)
    assert torch.equal(coef, want.float())                                      # formed in double, rounded ONCE: the same fp32 values
    u = 2.0 ** -24
    cy, cm = coef[:, 0].double(), coef[:, 1].double()
    assert bool(((cm[1:] - (1 - cy[1:])).abs() <= u * (1 + cy[1:].abs())).all())      # cm == 1 - cy to the rounding of both
    assert coef[0, 3].item() == 0.0
    if eta == 0.0:
        assert bool((coef[:, 3] == 0.0).all())
    elif len(tau) > 1:
        assert bool((coef[1:, 3] > 0.0).all())


def test_sampler_plan_refusals():
    from nested_diffusion_amd.diffusion_utils import sampler_plan
    _, omabs = ref_cpu.schedule_tables("linear", 20, 1e-4, 0.02)
    for eta in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError, match="eta"):
            sampler_plan(omabs, [0, 5], eta)
    for tau in ([], [3, 3], [5, 2], [-1, 4], [0, 20]):
        with pytest.raises(ValueError, match="timesteps"):
            sampler_plan(omabs, tau, 1.0)


# ---- eta = 1 is the reference's posterior on the derived tables -----------------------------------------------------------------------------
REFERENCE_CASES = [(20, 5, "uniform", False, 2e-5), (50, 10, "uniform", False, 2e-5), (1000, 20, "uniform", True, 2e-5),
                   (1000, 100, "uniform", True, 2e-5), (1000, 20, "quadratic", True, 5e-5)]


@pytest.mark.parametrize("T,S,skip_type,denoiser,bound", REFERENCE_CASES)
def test_eta_1_plan_against_the_references_arithmetic_on_the_derived_tables(T, S, skip_type, denoiser, bound):
    """The sub-chain tau is a DDPM chain of its own with tables omabs'_j = s[tau_j], alphas'_j = abar_{tau_j} / abar_{tau_{j-1}}.  The
    reference's fp32 posterior (ref_cpu.p_sample_given_eps / p_sample_t_1to0_given_eps, diffusion_utils.py:68-111) on those tables against
    the plan's coefficient form with the update in float64; both take eps from ref_cpu.trunk (fp32) at embedding row tau_j.  Bounds: the
    issue's, from its measured 2.5e-6 .. 4.7e-6 (uniform) and 1.9e-5 (quadratic; its early steps are consecutive timesteps, where the
    reference's own gamma expressions cancel hardest).  Contractive members at T = 1000: random weights amplify by ~160 there."""
    from nested_diffusion_amd.diffusion_utils import sampler_plan, timestep_sequence
    D, H, F, C, B = 64, 32, 64, 3, 5
    p = ref_cpu.init_cond_model_params(D, H, F, C, T, seed=3, denoiser=denoiser)
    _, omabs = ref_cpu.schedule_tables("linear", T, 1e-4, 0.02)
    tau = timestep_sequence(T, S, skip_type)
    n = len(tau)
    g = torch.Generator().manual_seed(11)
    x = torch.rand(B, D, generator=g)
    yhat = torch.softmax(torch.randn(B, C, generator=g), dim=1)
    z = torch.randn(n, B, C, generator=g)
    xe = ref_cpu.encoder_x(p, x)
    abar = 1.0 - omabs.double()[tau] ** 2
    omabs_d = omabs[tau].clone()
    alphas_d = torch.ones(n, dtype=torch.float64)
    alphas_d[1:] = abar[1:] / abar[:-1]
    alphas_d = alphas_d.float()
    # the reference's arithmetic, fp32
    y = z[0] + yhat
    for i, j in enumerate(range(n - 1, 0, -1), start=1):
        eps = ref_cpu.trunk(p, xe, y, torch.tensor([tau[j]]), yhat)
        y = ref_cpu.p_sample_given_eps(y, yhat, eps, j, alphas_d, omabs_d, z[i])
    eps = ref_cpu.trunk(p, xe, y, torch.tensor([tau[0]]), yhat)
    y_ref = ref_cpu.p_sample_t_1to0_given_eps(y, yhat, eps, omabs_d)
    # the coefficient form, update in float64
    coef = sampler_plan(omabs, tau, 1.0).coef.double()
    y = (z[0] + yhat).double()
    for i, j in enumerate(range(n - 1, 0, -1), start=1):
        eps = ref_cpu.trunk(p, xe, y.float(), torch.tensor([tau[j]]), yhat).double()
        y = coef[j, 0] * y + coef[j, 1] * yhat.double() + coef[j, 2] * eps + coef[j, 3] * z[i].double()
    eps = ref_cpu.trunk(p, xe, y.float(), torch.tensor([tau[0]]), yhat).double()
    y_coef = coef[0, 0] * y + coef[0, 1] * yhat.double() + coef[0, 2] * eps
    diff = float((y_ref.double() - y_coef).abs().max())
    print(f"T={T} S={n} {skip_type} denoiser={denoiser}: max |y_0 difference| {diff:.3e}, |y_0| max {float(y_ref.abs().max()):.3f}")
    assert float(y_ref.abs().max()) < 10.0                                      # a chain that does not amplify: the bound is absolute
    assert diff <= bound, diff


# ---- CLI ---------------------------------------------------------------------------------------------------------------------------------
BASE = ["--test", "--loss", "card_onehot_conditional", "--config", "none.yml", "--doc", "d", "--ni", "--preprocess", "grayscaled"]


def test_cli_reads_the_three_flags_only_with_sample_steps():
    from nested_diffusion_amd.main import build_parser
    from nested_diffusion_amd.runner import sampler_request
    parse = lambda *extra: build_parser().parse_args(BASE + list(extra))       # noqa: E731
    assert not hasattr(parse(), "sample_steps") and sampler_request(parse()) is None      # a flag that is not given leaves no attribute
    # without --sample_steps the three flags are parsed and ignored, whatever they say (as in the reference)
    assert sampler_request(parse("--skip_type", "nonsense", "--eta", "7", "--sample_type", "x")) is None
    assert sampler_request(argparse.Namespace(seed=1)) is None                 # a namespace that never heard of the flag
    assert sampler_request(parse("--sample_steps", "20")) == {"steps": 20, "skip_type": "uniform", "eta": 0.0}      # the reference's --eta default
    assert sampler_request(parse("--sample_steps", "20", "--eta", "0.5", "--skip_type", "quadratic")) == {"steps": 20, "skip_type": "quadratic", "eta": 0.5}
    assert sampler_request(parse("--sample_steps", "7", "--sample_type", "ddpm_noisy", "--eta", "0.25"))["eta"] == 1.0
    assert sampler_request(parse("--sample_steps", "7", "--timesteps", "100")) == {"steps": 7, "skip_type": "uniform", "eta": 0.0}


@pytest.mark.parametrize("extra,word", [(["--sample_steps", "0"], "--sample_steps"), (["--sample_steps", "-4"], "--sample_steps"),
                                        (["--sample_steps", "5", "--skip_type", "cosine"], "--skip_type"),
                                        (["--sample_steps", "5", "--sample_type", "ddim"], "--sample_type"),
                                        (["--sample_steps", "5", "--eta", "1.5"], "--eta"), (["--sample_steps", "5", "--eta", "-0.1"], "--eta")])
def test_cli_refuses_by_name_before_the_gpu_is_touched(extra, word, monkeypatch):
    """main() refuses right after parsing: before the config file is opened, a process group is joined or a device is picked (the config
    named here does not exist, and torch.cuda is made to raise if it is asked)."""
    import nested_diffusion_amd.main as nd_main
    from nested_diffusion_amd.runner import sampler_request

    def boom(*a, **k):
        raise AssertionError("the GPU was asked")
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    with pytest.raises(SystemExit) as e:
        nd_main.main(BASE + extra)
    assert word in str(e.value)
    with pytest.raises(ValueError, match=word):
        sampler_request(nd_main.build_parser().parse_args(BASE + extra))


def test_runner_builds_the_plan_from_args_and_counts_its_steps():
    """Diffusion.__init__ is host work up to the conditioner: with --sample_steps it holds the plan, and S is what predict_batch / the
    throughput line / draw_noise use; without, nothing changes."""
    from nested_diffusion_amd.diffusion_utils import sampler_plan, timestep_sequence
    from nested_diffusion_amd.runner import Diffusion
    ns = argparse.Namespace
    cfg = ns(data=ns(dataset="ChestXRay", num_classes=2), model=ns(data_dim=48, hidden_dim=16, feature_dim=16),
             diffusion=ns(timesteps=1000, beta_schedule="linear", beta_start=1e-4, beta_end=0.02, aux_cls=ns(arch="sevit")))
    cond = ns(mlps=[None] * 3)
    plain = Diffusion(ns(seed=1, skip_type="quadratic", eta=0.3), cfg, device="cpu", conditioner=cond)
    assert plain.plan is None and plain.sampler is None and plain.sample_steps == 1000
    r = Diffusion(ns(seed=1, sample_steps=20, skip_type="quadratic", eta=0.5, sample_type="generalized"), cfg, device="cpu", conditioner=cond)
    tau = timestep_sequence(1000, 20, "quadratic")
    want = sampler_plan(r.one_minus_alphas_bar_sqrt, tau, 0.5)
    assert r.sample_steps == len(tau) == 20 and r.num_timesteps == 1000
    assert torch.equal(r.plan.timesteps, want.timesteps) and torch.equal(r.plan.coef, want.coef)
    with pytest.raises(ValueError, match="--eta"):
        Diffusion(ns(seed=1, sample_steps=20, eta=2.0), cfg, device="cpu", conditioner=cond)


def test_make_attacks_flags_and_refusals():
    from nested_diffusion_amd.make_attacks import build_parser, sampler_args
    base = ["--config", "c.yml", "--attack_name", "PGD", "--eps", "0.03", "--out", "o"]
    parse = lambda *extra: build_parser().parse_args(base + list(extra))       # noqa: E731
    assert sampler_args(parse()) == {} and sampler_args(parse("--target", "ensemble")) == {}
    assert sampler_args(parse("--target", "ensemble", "--sample_steps", "10")) == {"sample_steps": 10, "skip_type": "uniform", "eta": 1.0}
    assert sampler_args(parse("--target", "ensemble", "--sample_steps", "10", "--skip_type", "quadratic", "--eta", "0")) == \
        {"sample_steps": 10, "skip_type": "quadratic", "eta": 0.0}
    for extra, word in ((["--sample_steps", "10"], "--target ensemble"), (["--target", "conditioner", "--sample_steps", "10"], "--target ensemble"),
                        (["--target", "ensemble", "--eta", "0.5"], "--eta"), (["--target", "ensemble", "--skip_type", "uniform"], "--skip_type"),
                        (["--target", "ensemble", "--sample_steps", "0"], "--sample_steps"),
                        (["--target", "ensemble", "--sample_steps", "4", "--skip_type", "x"], "--skip_type"),
                        (["--target", "ensemble", "--sample_steps", "4", "--eta", "1.2"], "--eta")):
        with pytest.raises(SystemExit) as e:
            sampler_args(parse(*extra))
        assert word in str(e.value), (extra, str(e.value))


def test_tape_and_target_signatures_take_the_plan():
    import inspect
    from nested_diffusion_amd import diffusion_utils, engine, ensemble_grad
    tape = inspect.signature(ensemble_grad.SamplerTape.__init__).parameters
    assert tape["timesteps"].default is None and tape["eta"].default == 1.0
    tgt = inspect.signature(ensemble_grad.EnsembleTarget.__init__).parameters
    assert tgt["sample_steps"].default is None and tgt["skip_type"].default == "uniform" and tgt["eta"].default == 1.0
    loop = inspect.signature(diffusion_utils.p_sample_loop).parameters
    assert loop["timesteps"].default is None and loop["eta"].default == 1.0
    assert hasattr(engine.EnsembleEngine, "set_sampler") and hasattr(engine.EnsembleEngine, "clear_sampler")


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_header_library_and_ctypes_table_carry_the_entry_points():
    from nested_diffusion_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "nested_diffusion.h")).read()
    for name, n_args in SYMBOLS.items():
        decl = re.search(rf"\bint {name}\(([^;]*)\);", header)
        assert decl, name
        assert len([a for a in decl.group(1).split(",") if a.strip()]) == n_args, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args, name
    lib = ctypes.CDLL(build.build())
    for name in SYMBOLS:
        assert hasattr(lib, name), name


def _refused(rc, lib, *words):
    msg = lib.nd_last_error().decode()
    assert rc == -1, (rc, msg)                                                  # ND_ERR_ARG
    for w in words:
        assert w in msg, (w, msg)


def test_nd_set_sampler_validates_its_arguments_without_a_gpu():
    """Every case is refused before anything is allocated, copied or launched (there is no device here); a refused call leaves the
    handle without a plan, and clearing a plan that is not there is fine."""
    from nested_diffusion_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.nd_create(ctypes.byref(_lib.NdConfig(2, 48, 64, 64, 10, 1, 4, 4)), ctypes.byref(h)) == 0       # n_steps = 10
    i32, f32 = ctypes.c_int32, ctypes.c_float
    tau = lambda *v: (i32 * len(v))(*v)                                         # noqa: E731
    co = lambda n, **bad: (f32 * (4 * n))(*[bad.get(f"at{k}", 0.5) for k in range(4 * n)])     # noqa: E731
    st = lib.nd_set_sampler
    _refused(st(None, tau(0, 1), co(2), 2, None), lib, "handle is NULL")
    _refused(st(h, tau(0, 1), co(2), -1, None), lib, "S=-1 outside [0,10]")
    _refused(st(h, tau(*range(11)), co(11), 11, None), lib, "S=11 outside [0,10]")
    _refused(st(h, None, co(2), 2, None), lib, "NULL")
    _refused(st(h, tau(0, 1), None, 2, None), lib, "NULL")
    _refused(st(h, tau(0, 10), co(2), 2, None), lib, "timesteps[1]=10 outside [0,10)")
    _refused(st(h, tau(-1, 3), co(2), 2, None), lib, "timesteps[0]=-1 outside [0,10)")
    _refused(st(h, tau(3, 3), co(2), 2, None), lib, "strictly increasing", "timesteps[1]=3")
    _refused(st(h, tau(2, 5, 4), co(3), 3, None), lib, "strictly increasing", "timesteps[2]=4")
    _refused(st(h, tau(2, 5), co(2, at6=float("nan")), 2, None), lib, "coefficient [1][2] is not finite")
    _refused(st(h, tau(2, 5), co(2, at3=float("inf")), 2, None), lib, "coefficient [0][3] is not finite")
    assert lib.nd_sampler_steps(h) == 0 and lib.nd_sampler_steps(None) == 0
    assert st(h, None, None, 0, None) == 0 and lib.nd_sampler_steps(h) == 0     # S = 0 clears; the pointers are not read
    assert lib.nd_loop_form(h) == 0
    rc = lib.nd_reverse_step_coef
    P = 0x10000
    _refused(rc(None, 4, P, P, P, P + 4096, 4, 6, 3, 4, 1.0, 0.0, 0.0, 0.0, None), lib, "NULL")
    _refused(rc(P, 4, P, P, None, P + 4096, 4, 6, 3, 4, 1.0, 0.0, 0.0, 0.5, None), lib, "cz=0.5 needs the draw z")
    _refused(rc(P, 4, P, P, P, P + 4096, 4, 6, 3, 4, float("nan"), 0.0, 0.0, 0.0, None), lib, "not finite")
    _refused(rc(P, 4, P, P, P, P + 4096, 4, 7, 3, 4, 1.0, 0.0, 0.0, 0.0, None), lib, "M % B == 0")
    _refused(rc(P, 4, P, P, P, P + 4096, 4, 6, 3, 9, 1.0, 0.0, 0.0, 0.0, None), lib, "C <= 8")
    _refused(rc(P, 4, P, P, P, P + 4096, 5, 6, 3, 4, 1.0, 0.0, 0.0, 0.0, None), lib, "ldo must be C or in [2C, 64]")
    _refused(rc(P, 3, P, P, P, P + 4096, 4, 6, 3, 4, 1.0, 0.0, 0.0, 0.0, None), lib, "ldy must lie in [C, 64]")
    _refused(rc(P, 4, P, P, P, P, 4, 6, 3, 4, 1.0, 0.0, 0.0, 0.0, None), lib, "out aliases an input")
    assert lib.nd_destroy(h) == 0
