"""Host-side checks of the conditioner input gradient (no GPU): the ABI carries nd_linear_bwd and nd_ensemble_xent_bwd, ConditionerTarget is
not unwrapped by the attacks, Carlini-Wagner on a target refuses by name, make_attacks' defaults are unchanged, and the ensemble head's
closed form (restated here in float32, in the kernel's order) agrees with float64 autograd."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nd_linear_bwd", "nd_ensemble_xent_bwd")


def test_header_lib_signatures_and_library_carry_both_entry_points():
    from nested_diffusion_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "nested_diffusion.h")).read()
    for name in SYMBOLS:
        decl = re.search(rf"\bint {name}\(([^;]*)\);", header)
        assert decl, name
        n_args = len([a for a in decl.group(1).split(",") if a.strip()])
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args
    assert "#define ND_LINEAR_BWD_MAX_M 128" in header
    assert "nd_mlp_grad.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "nd_mlp_grad.hip"))
    lib = ctypes.CDLL(build.build())
    for name in SYMBOLS:
        assert hasattr(lib, name), name


class _FakeVit:
    device = torch.device("cpu")


class _FakeCond:
    def __init__(self, K=3):
        self.vit, self.mlps = _FakeVit(), [object()] * K

    def _members(self, members):
        from nested_diffusion_amd.mapping import GuidingConditioner
        return GuidingConditioner._members(self, members)


def test_conditioner_target_is_not_unwrapped_and_cw_refuses_by_name():
    from nested_diffusion_amd import attack, autoattack
    from nested_diffusion_amd.mapping import ConditionerTarget
    target = ConditionerTarget(_FakeCond(), members=[0, 2])
    assert not hasattr(target, "vit") and attack._vit(target) is target
    assert target.members == [0, 2] and target.device == torch.device("cpu") and isinstance(target.cond, _FakeCond)
    assert ConditionerTarget(_FakeCond()).members is None
    assert attack.Attack(0.1, "PGD", target).model is target
    assert attack.L2Attack(0.1, "L2PGD", target).model is target
    assert autoattack.AutoAttack(target, eps=0.1, version="custom", attacks_to_run=["apgd-ce"]).model is target
    with pytest.raises(NotImplementedError, match="Carlini"):
        target.input_grad_margin(None, None, None)
    with pytest.raises(NotImplementedError, match="Carlini"):
        attack.CarliniWagner(0.1, target)
    with pytest.raises(NotImplementedError, match="Carlini"):
        attack.make_attack(0.1, "CW", target)
    for bad in ([], [0, 0], [3], [-1]):
        with pytest.raises(ValueError):
            ConditionerTarget(_FakeCond(), members=bad)


def test_make_attacks_parser_defaults_are_unchanged():
    from nested_diffusion_amd import make_attacks
    a = make_attacks.build_parser().parse_args(["--config", "c.yml", "--attack_name", "PGD", "--eps", "0.03", "--out", "o"])
    assert vars(a) == {"config": "c.yml", "attack_name": "PGD", "eps": 0.03, "out": "o", "preprocess": "grayscaled", "seed": 0,
                       "batch_size": 32, "dataroot": None, "device": 0, "target": "vit", "members": None}
    b = make_attacks.build_parser().parse_args(["--config", "c.yml", "--attack_name", "FGSM", "--eps", "1", "--out", "o", "--target",
                                                "conditioner", "--members", "0,2"])
    assert b.target == "conditioner" and make_attacks.parse_members(b.members) == [0, 2] and make_attacks.parse_members(None) is None
    with pytest.raises(SystemExit):
        make_attacks.build_parser().parse_args(["--config", "c", "--attack_name", "PGD", "--eps", "1", "--out", "o", "--target", "head"])
    with pytest.raises(SystemExit, match="--members"):             # members of the ViT head: refused before anything is read
        make_attacks.main(["--config", "/nonexistent.yml", "--attack_name", "PGD", "--eps", "1", "--out", "o", "--members", "0"])


def test_make_attacks_checkpoint_name():
    import types
    from nested_diffusion_amd import make_attacks
    cfg = lambda ds: types.SimpleNamespace(data=types.SimpleNamespace(dataset=ds))   # noqa: E731
    assert make_attacks.checkpoint_name(cfg("ChestXRay")) == make_attacks.checkpoint_name(cfg("ChestXRayAtkFGSM")) == "ChestXRay"
    assert make_attacks.checkpoint_name(cfg("ISICSkinCancerValidate")) == "ISICSkinCancer"


def ensemble_head_f32(logits: torch.Tensor, labels: torch.Tensor):
    """nd_ensemble_xent_bwd restated in float32: (P, loss, dlogits)."""
    K, B, C = logits.shape
    e = torch.exp(logits - logits.max(dim=2, keepdim=True).values)
    p = e / e.sum(dim=2, keepdim=True)
    P = torch.zeros(B, C)
    for k in range(K):
        P = P + p[k]
    P = P / K
    py = p[:, torch.arange(B), labels]                     # [K, B]
    S = torch.zeros(B)
    for k in range(K):
        S = S + py[k]
    loss = -torch.log(S / K)
    onehot = torch.nn.functional.one_hot(labels, C).float()
    return P, loss, (py / S)[:, :, None] * (p - onehot)


@pytest.mark.parametrize("K,C", [(1, 2), (3, 3), (5, 7), (32, 64)])
def test_ensemble_head_closed_form_agrees_with_float64_autograd(K, C):
    g = torch.Generator().manual_seed(100 * K + C)
    B = 5
    logits = torch.randn(K, B, C, generator=g) * 3
    labels = torch.randint(0, C, (B,), generator=g)
    l64 = logits.double().requires_grad_(True)
    P64 = torch.softmax(l64, dim=2).mean(dim=0)
    loss64 = -torch.log(P64[torch.arange(B), labels])
    loss64.sum().backward()
    P, loss, d = ensemble_head_f32(logits, labels)
    rel = lambda a, b: float((a.double() - b).norm() / b.norm())   # noqa: E731
    assert rel(P, P64.detach()) <= 1e-6 and rel(loss, loss64.detach()) <= 1e-6 and rel(d, l64.grad) <= 1e-6
    # the closed form itself, in float64, is autograd's gradient to rounding
    p64 = torch.softmax(logits.double(), dim=2)
    py = p64[:, torch.arange(B), labels]
    d64 = (py / py.sum(0))[:, :, None] * (p64 - torch.nn.functional.one_hot(labels, C).double())
    assert float((d64 - l64.grad).abs().max()) <= 1e-14
