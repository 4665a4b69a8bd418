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
    onehot = torch.nn.functional.one_hot(labels, C).float()
    if K == 1:                                             # the plain cross-entropy, a log-softmax: no division by p_y, no underflow to report
        mx = logits[0].max(dim=1).values
        loss = torch.log(e[0].sum(dim=1)) - (logits[0, torch.arange(B), labels] - mx)
        return P, loss, p - onehot
    loss = -torch.log(S / K)
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


@pytest.mark.parametrize("C", [2, 10, 1000])
@pytest.mark.parametrize("margin", [0, 5, 15, 20, 40, 80, 90, 103, 110])
def test_one_member_is_torch_cross_entropy_at_confident_logits(margin, C):
    """K = 1 (the trainer's loss head) on rows that lead with the label by `margin` and rows where another class leads it by `margin`: the
    float32 restatement stays within 4 * 2^-24 * max(1, max |logit|) of float64 F.cross_entropy and within a few ulps of p (of 1 at the
    label) of softmax - onehot (torch's float32, and float64 once the shared rounding of l - max is counted), past the margin of 104 where exp(l_y - max) is 0 in fp32 -- there the loss is the margin and the gradient at
    the label -1.  The ensemble form -log(p_y), (p_y / p_y) (p - onehot) gives +inf and 0 / 0 there."""
    B, U24 = 16, 2.0 ** -24
    g = torch.Generator().manual_seed(margin * 100 + C)
    logits = 8 + 0.5 * torch.randn(B, C, generator=g)
    labels = torch.randint(0, C, (B,), generator=g)
    rows = torch.arange(B)
    logits[rows[: B // 2], labels[: B // 2]] = (logits.max(1).values + margin)[: B // 2]
    other = (labels[B // 2:] + 1) % C
    logits[rows[B // 2:], other] = logits[rows[B // 2:], labels[B // 2:]] + margin
    _, loss, d = ensemble_head_f32(logits[None], labels)
    l64 = logits.double()
    onehot = torch.nn.functional.one_hot(labels, C).double()
    p64 = torch.softmax(l64, 1)
    want = torch.nn.functional.cross_entropy(l64, labels, reduction="none")
    assert bool(((loss.double() - want).abs() <= 4 * U24 * l64.abs().max(1).values.clamp(min=1)).all())
    # the elementwise bound of test_xent_head_grad_confident_logits, against torch's float32 softmax as there; against float64 the rounding of
    # l_c - max (|l_c - max| 2^-24, relative in p_c), which every fp32 softmax shares, joins it
    p32 = torch.softmax(logits, 1).double()
    ulps = 2 * (-(-C // 64) + 8) * U24 * (p32 + onehot) + 2.0 ** -126
    assert bool(((d[0].double() - (p32 - onehot)).abs() <= ulps).all())
    arg = (l64 - l64.max(1, keepdim=True).values).abs() * U24 * p64
    assert bool(((d[0].double() - (p64 - onehot)).abs() <= ulps + arg).all())
    if margin >= 103:
        wrong = rows[B // 2:]
        assert bool(((loss[wrong].double() - margin).abs() <= 2.0 ** -15).all()) and bool((d[0, wrong, labels[wrong]] == -1).all())
        e_y = torch.exp(logits[wrong, labels[wrong]] - logits[wrong].max(1).values)
        if margin >= 110:
            assert bool((e_y == 0).all())                  # what the ensemble form divides by
