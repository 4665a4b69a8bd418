"""Host-side checks of the input gradient through the sampler (no GPU): the ABI carries the six entry points of csrc/nd_ensemble_grad.hip,
the reverse-step coefficients agree with float64 autograd through the oracle's p_sample, the folded tables are the oracle's eval BatchNorm,
make_attacks takes --target ensemble, and EnsembleTarget refuses its bad arguments before anything is packed or launched."""
import ctypes
import os
import re
import types

import pytest
import torch

from oracle import ref_cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nd_cond_mul", "nd_cond_act_bwd", "nd_reverse_step", "nd_reverse_step_bwd", "nd_aggregate_xent_bwd", "nd_softmax_bwd")
U24 = 2.0 ** -24


def test_header_lib_signatures_and_library_carry_the_entry_points():
    from nested_diffusion_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "nested_diffusion.h")).read()
    for name in SYMBOLS:
        decl = re.search(rf"\bint {name}\(([^;]*)\);", header)
        assert decl, name
        n_args = len([a for a in decl.group(1).split(",") if a.strip()])
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args, name
    for define in ("#define ND_RSTEP_INIT 0", "#define ND_RSTEP_UPDATE 1", "#define ND_RSTEP_LAST 2"):
        assert define in header
    assert "nd_ensemble_grad.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "nd_ensemble_grad.hip"))
    lib = ctypes.CDLL(build.build())
    for name in SYMBOLS:
        assert hasattr(lib, name), name


@pytest.mark.parametrize("T", [1, 2, 10, 1000])
def test_reverse_step_coefficients_agree_with_float64_autograd(T):
    """(cy, cm, ce) at t in {0, 1, T - 1} against autograd through ref_cpu.p_sample_given_eps / p_sample_t_1to0_given_eps on the fp32 tables
    converted to double: the function forms them in double and stores them as fp32, so |c - c64| <= 2^-24 |c64| (one round-to-nearest store)
    plus 1e-13 for the double evaluation itself."""
    from nested_diffusion_amd.ensemble_grad import reverse_step_coefficients
    alphas, omabs = ref_cpu.schedule_tables("linear", T, 1e-4, 0.02)
    coef = reverse_step_coefficients(alphas, omabs)
    assert coef.dtype == torch.float32 and tuple(coef.shape) == (T, 3)
    a64, s64 = alphas.double(), omabs.double()
    g = torch.Generator().manual_seed(T)
    for t in sorted({0, 1, T - 1}):
        if t >= T:
            continue
        y, ym, eps = (torch.randn(3, 2, generator=g, dtype=torch.float64).requires_grad_(True) for _ in range(3))
        if t == 0:
            out = ref_cpu.p_sample_t_1to0_given_eps(y, ym, eps, s64)
        else:
            out = ref_cpu.p_sample_given_eps(y, ym, eps, t, a64, s64, torch.zeros(3, 2, dtype=torch.float64))
        out.sum().backward()
        for got, grad, name in zip(coef[t].tolist(), (y.grad, ym.grad, eps.grad), ("cy", "cm", "ce")):
            want = float(grad[0, 0])
            assert float((grad - want).abs().max()) <= 1e-13 * max(1.0, abs(want))     # the step is affine: one number per operand
            assert abs(got - want) <= U24 * abs(want) + 1e-13, (T, t, name, got, want)
    with pytest.raises(ValueError):
        reverse_step_coefficients(alphas, omabs[:-1] if T > 1 else torch.zeros(0))


def test_folded_tables_are_the_oracles_eval_batchnorm():
    """a_t (W h) + c_t against ref_cpu's Linear -> per-timestep gain -> eval BatchNorm in float64: the fold is formed in double and stored
    as fp32, so the two agree to the fp32 rounding of a_t and c_t."""
    from nested_diffusion_amd.ensemble_grad import _fold
    T, F = 5, 48
    p = ref_cpu.init_cond_model_params(64, 32, F, 3, T, seed=2)
    u = torch.randn(7, F, generator=torch.Generator().manual_seed(1), dtype=torch.float64)          # W h, before the bias
    p64 = {k: v.double() for k, v in p.items()}
    a, c = _fold(p, "lin2.lin", "unetnorm2", "lin2.embed.weight", T)
    assert tuple(a.shape) == tuple(c.shape) == (T, F) and a.dtype == torch.float32
    for t in range(T):
        want = ref_cpu._bn_eval(p64["lin2.embed.weight"][t] * (u + p64["lin2.lin.bias"]), p64, "unetnorm2")
        got = a[t].double() * u + c[t].double()
        assert float((got - want).abs().max()) <= 4 * U24 * float(want.abs().max())
    a, c = _fold(p, "encoder_x.6", "norm", None, T)
    assert tuple(a.shape) == (1, F)
    want = ref_cpu._bn_eval(u + p64["encoder_x.6.bias"], p64, "norm")
    assert float((a[0].double() * u + c[0].double() - want).abs().max()) <= 4 * U24 * float(want.abs().max())


def test_make_attacks_parser_takes_the_ensemble_target():
    from nested_diffusion_amd import make_attacks
    base = ["--config", "c.yml", "--attack_name", "PGD", "--eps", "0.03", "--out", "o"]
    a = make_attacks.build_parser().parse_args(base)
    assert "mc" not in vars(a) and a.target == "vit"                      # a new option leaves the default parse as it was
    b = make_attacks.build_parser().parse_args(base + ["--target", "ensemble", "--members", "0,2", "--mc", "3"])
    assert b.target == "ensemble" and b.mc == 3 and make_attacks.parse_members(b.members) == [0, 2]
    assert callable(make_attacks.load_ensemble_target)
    with pytest.raises(SystemExit, match="--mc"):                          # trials of the ViT head: refused before anything is read
        make_attacks.main(["--config", "/nonexistent.yml", "--attack_name", "PGD", "--eps", "1", "--out", "o", "--mc", "2"])


class _FakeVit:
    device = torch.device("cpu")
    dtype, split = "f32", True


class _FakeCond:
    def __init__(self, K=3, dtype="f32"):
        self.vit, self.mlps = _FakeVit(), [object()] * K
        self.vit.dtype = dtype

    def _members(self, members):
        from nested_diffusion_amd.mapping import GuidingConditioner
        return GuidingConditioner._members(self, members)


def _config(T=4, C=2, D=64, H=32, F=48):
    ns = types.SimpleNamespace
    return ns(data=ns(dataset="ChestXRay", num_classes=C), model=ns(data_dim=D, hidden_dim=H, feature_dim=F),
              diffusion=ns(timesteps=T, beta_schedule="linear", beta_start=1e-4, beta_end=0.02))


def test_ensemble_target_refuses_bad_arguments_without_a_gpu(monkeypatch):
    from nested_diffusion_amd import _lib
    from nested_diffusion_amd.ensemble_grad import EnsembleTarget, check_call, member_dims
    states = [ref_cpu.init_cond_model_params(64, 32, 48, 2, 4, seed=k) for k in range(3)]
    with pytest.raises(_lib.NdError, match="fp16"):
        EnsembleTarget(_FakeCond(dtype="f16"), states, _config())
    monkeypatch.setenv("ND_GEMM_F32", "mfma_f32")
    with pytest.raises(_lib.NdError, match="mfma_f32"):
        EnsembleTarget(_FakeCond(), states, _config())
    monkeypatch.delenv("ND_GEMM_F32")
    with pytest.raises(ValueError, match="mc"):
        EnsembleTarget(_FakeCond(), states, _config(), mc=0)
    for bad in ([], [0, 0], [3], [-1]):
        with pytest.raises(ValueError):
            EnsembleTarget(_FakeCond(), states, _config(), members=bad)
    with pytest.raises(ValueError, match="no noise estimator state"):     # member 2 has an MLP and no state
        EnsembleTarget(_FakeCond(), states[:2], _config(), members=[0, 2])
    with pytest.raises(ValueError, match="temperature"):
        EnsembleTarget(_FakeCond(), states, _config(), temperature=0.0)
    with pytest.raises(ValueError, match="config says"):                   # the states are not the config's shapes
        EnsembleTarget(_FakeCond(), states, _config(F=64), temperature=0.25)
    with pytest.raises(ValueError, match="timesteps"):                     # more timesteps than embedding rows
        EnsembleTarget(_FakeCond(), states, _config(T=9), temperature=0.25)
    # the per-call refusals
    assert check_call(32, 4, 3, 4, 2, (3, 4, 128, 2)) == 128 and check_call(1, 1, 1, 1, 2, None) == 1
    with pytest.raises(ValueError, match="128"):
        check_call(33, 4, 3, 4, 2, None)
    for shape in ((3, 4, 64, 2), (2, 4, 128, 2), (3, 5, 128, 2), (3, 4, 128, 3), (3, 4, 128)):
        with pytest.raises(ValueError, match="noise"):
            check_call(32, 4, 3, 4, 2, shape)
    # a member's shapes
    assert member_dims(states[0]) == (2, 64, 32, 48, 4)
    with pytest.raises(ValueError, match="multiples of 16"):
        member_dims(ref_cpu.init_cond_model_params(72, 32, 48, 2, 4))
    with pytest.raises(ValueError, match="num_classes"):
        member_dims(ref_cpu.init_cond_model_params(64, 32, 48, 9, 4))
    with pytest.raises(ValueError, match="guidance"):
        member_dims(ref_cpu.init_cond_model_params(64, 32, 48, 2, 4, guidance=False))
    with pytest.raises(KeyError):
        member_dims({k: v for k, v in states[0].items() if k != "norm.weight"})


def test_member_layout_is_the_reference_models():
    """latent_model's layout of the noise estimator -- what the trainer and the ensemble gradient both hold their members by -- against
    the module it describes, built on the CPU."""
    import struct
    from nested_diffusion_amd import ensemble_grad, latent_model, ops, train_diffusion
    C, D, H, F, T = 2, 32, 16, 16, 3
    ns = types.SimpleNamespace
    config = ns(data=ns(dataset="ChestXRay", num_classes=C), model=ns(data_dim=D, hidden_dim=H, feature_dim=F, arch="linear"),
                diffusion=ns(timesteps=T))
    model = latent_model.ConditionalModel(config, guidance=True)
    params = {k: tuple(p.shape) for k, p in model.named_parameters()}
    table = latent_model.member_shapes(C, D, H, F, T)
    assert table == params and list(table) == list(params) == list(train_diffusion.PARAM_KEYS)     # key for key, in registration order
    assert latent_model.LIN1_K == 16 and train_diffusion.LIN1_K is latent_model.LIN1_K and ensemble_grad.LIN1_K is latent_model.LIN1_K
    assert ensemble_grad.BN_EPS == ops.BN_EPS == model.norm.eps
    latent_model.check_member_dims(C, D, H, F, T)
    with pytest.raises(ValueError, match="multiples of 16"):
        latent_model.check_member_dims(C, 24, H, F, T)
    with pytest.raises(ValueError, match="num_classes"):
        latent_model.check_member_dims(9, D, H, F, T)
    with pytest.raises(ValueError, match="T=0"):
        latent_model.check_member_dims(C, D, H, F, 0)
    w = torch.randn(F, 2 * C, generator=torch.Generator().manual_seed(1))
    w[0, 0] = -0.0
    padded = latent_model.pad_lin1(w)
    assert tuple(padded.shape) == (F, 16) and padded.dtype == torch.float32 and padded.is_contiguous()
    assert padded[:, :2 * C].contiguous().numpy().tobytes() == w.numpy().tobytes()
    assert padded[:, 2 * C:].contiguous().numpy().tobytes() == struct.pack("<f", 0.0) * (F * (16 - 2 * C))      # +0.0, bit for bit


def test_ensemble_target_is_not_unwrapped_and_cw_refuses_by_name():
    from nested_diffusion_amd import attack
    from nested_diffusion_amd.ensemble_grad import EnsembleTarget
    target = object.__new__(EnsembleTarget)                               # the duck type alone: nothing is packed
    target.device = torch.device("cpu")
    assert not hasattr(target, "vit") and attack._vit(target) is target
    assert attack.Attack(0.1, "PGD", target).model is target and attack.L2Attack(0.1, "L2PGD", target).model is target
    with pytest.raises(NotImplementedError, match="Carlini"):
        target.input_grad_margin(None, None, None)
    with pytest.raises(NotImplementedError, match="Carlini"):
        attack.CarliniWagner(0.1, target)
    with pytest.raises(NotImplementedError, match="Carlini"):
        attack.make_attack(0.1, "CW", target)
