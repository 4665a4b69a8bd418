"""Host-side pieces of the L2 attacks and Carlini & Wagner: the attack table, the make_attack factory, the defaults, the C ABI
declarations and argument checks of the new entry points, make_attacks' parser and apply_attack's dispatch (no GPU needed)."""
import math
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["nd_margin_head_bwd", "nd_l2_step", "nd_l2_random_start", "nd_cw_attack_space", "nd_cw_model_space", "nd_cw_control",
               "nd_cw_update"]
FAKE = types.SimpleNamespace(device="cpu")


def test_l2_attack_table():
    from nested_diffusion_amd import attack
    want = {"BIM": ("L2BasicIterativeAttack", 0.2, 10, False), "L2PGD": ("L2ProjectedGradientDescentAttack", 0.025, 50, True)}
    assert attack.L2_ATTACKS == want
    for name, (_, rel, steps, rs) in want.items():
        a = attack.L2Attack(2.0, name, FAKE, seed=5)
        assert (a.attack_type, a.steps, a.random_start, a.seed) == (name, steps, rs, 5)
        assert math.isclose(a.stepsize, rel * 2.0)
    assert attack.L2Attack(0.5, "BIM", types.SimpleNamespace(vit=FAKE)).model is FAKE
    for bad in ("FGSM", "CW", "Nope"):
        with pytest.raises(ValueError):
            attack.L2Attack(0.5, bad, FAKE)


def test_make_attack_knows_the_six_names():
    from nested_diffusion_amd import attack
    kinds = {"FGSM": attack.Attack, "PGD": attack.Attack, "LinfBIM": attack.Attack, "BIM": attack.L2Attack, "L2PGD": attack.L2Attack,
             "CW": attack.CarliniWagner}
    for name, cls in kinds.items():
        a = attack.make_attack(0.3, name, FAKE, seed=2)
        assert type(a) is cls and a.attack_type == name and a.epsilon == 0.3 and a.model is FAKE
    for bad in ("AUTOPGD", "Nope", ""):
        with pytest.raises(ValueError):
            attack.make_attack(0.3, bad, FAKE)


def test_carlini_wagner_defaults_are_the_reference_call():
    from nested_diffusion_amd import attack
    a = attack.CarliniWagner(1.5, FAKE)
    assert (a.binary_search_steps, a.steps, a.stepsize, a.confidence, a.initial_const, a.abort_early) == (6, 1000, 0.01, 0.0, 1e-3, True)
    assert a.attack_type == "CW" and a.epsilon == 1.5
    m = attack.make_attack(1.5, "CW", FAKE)
    assert (m.binary_search_steps, m.steps, m.stepsize, m.confidence) == (6, 1000, 0.01, 0.0)


def test_header_signatures_ops_and_sources_carry_the_new_entry_points():
    from nested_diffusion_amd import _lib, build, ops
    with open(os.path.join(ROOT, "include", "nested_diffusion.h")) as f:
        hdr = f.read()
    for s in NEW_SYMBOLS:
        assert re.search(rf"\bint {s}\(", hdr), s
        assert s in _lib.SIGNATURES, s
    for w in ("margin_head_grad", "l2_step", "l2_random_start", "cw_attack_space", "cw_model_space", "cw_control", "cw_update"):
        assert callable(getattr(ops, w)), w
    m = re.search(r"#define ND_L2_START_TAG (0x[0-9A-Fa-f]+)u", hdr)
    assert m and int(m.group(1), 16) not in (0x41544B31, 0x41504731)          # distinct from the Linf and APGD tags
    assert f"#define ND_L2_MAX_PARTS {ops.L2_MAX_PARTS}\n" in hdr
    assert "nd_attack_l2.hip" in build.SOURCES
    from nested_diffusion_amd.mapping import VisionTransformer
    assert callable(VisionTransformer.input_grad_margin)


def test_new_entry_points_refuse_bad_arguments_before_any_launch():
    """ND_ERR_ARG with an nd_last_error text before any HIP call (dummy non-NULL pointers: nothing is dereferenced)."""
    from nested_diffusion_amd import _lib, build
    build.build()
    lib = _lib.load()
    P = 4096                                                       # a dummy non-NULL, 16-byte aligned address, never dereferenced
    rows = rb"1 <= B <= 65535 and per_image % 4 == 0"
    cases = []
    for B, per in ((2, 6), (0, 8), (65536, 8), (2, 0)):
        cases += [
            (lambda B=B, per=per: lib.nd_l2_step(P, P, P, P, P, P, P, B, per, 0.1, 1.0, 0.0, 1.0, None), rb"l2 step needs " + rows),
            (lambda B=B, per=per: lib.nd_l2_random_start(P, P, P, P, B, per, 1, 0, 0, 1.0, 0.0, 1.0, None), rb"l2 random start needs " + rows),
            (lambda B=B, per=per: lib.nd_cw_model_space(P, P, P, P, P, P, P, P, P, B, per, 0.0, 1.0, None), rb"cw model space needs " + rows),
            (lambda B=B, per=per: lib.nd_cw_update(P, P, P, P, P, P, P, P, P, B, per, 0.01, 0.1, 0.001, 0.5, None), rb"cw update needs " + rows),
        ]
    cases += [
        (lambda: lib.nd_cw_attack_space(P, P, P, 6, 0.0, 1.0, None), rb"n % 4 == 0"),
        (lambda: lib.nd_cw_attack_space(P, P, P, 0, 0.0, 1.0, None), rb"n % 4 == 0"),
        (lambda: lib.nd_cw_attack_space(P, P, P, 8, 1.0, 1.0, None), rb"lo < hi"),
        (lambda: lib.nd_l2_step(P, P, P, P + 4, P, P, P, 2, 8, 0.1, 1.0, 0.0, 1.0, None), rb"16-byte aligned"),
        (lambda: lib.nd_l2_step(P, P, P, P, None, P, P, 2, 8, 0.1, 1.0, 0.0, 1.0, None), rb"NULL tensor"),
        (lambda: lib.nd_margin_head_bwd(P, P, P, P, P, P, P, 2, 1, 768, 0.0, None), rb"2 <= C <= 1024 \(C=1\)"),
        (lambda: lib.nd_margin_head_bwd(P, P, P, P, P, P, P, 2, 1025, 768, 0.0, None), rb"2 <= C <= 1024 \(C=1025\)"),
        (lambda: lib.nd_cw_control(P, P, P, P, P, P, P, P, P, P, 2, 1, 0.0, None), rb"2 <= C <= 1024 \(B=2, C=1\)"),
        (lambda: lib.nd_cw_control(P, P, P, P, P, P, P, P, P, P, 2, 1025, 0.0, None), rb"2 <= C <= 1024"),
        (lambda: lib.nd_cw_control(P, P, P, P, P, P, P, P, P, P, 0, 2, 0.0, None), rb"1 <= B <= 65535"),
        (lambda: lib.nd_cw_control(P, P, P, P, P, P, P, P, P, P, 65536, 2, 0.0, None), rb"1 <= B <= 65535"),
    ]
    # one misaligned image pointer per call, everything else valid: each position of each entry point that reads or writes float4
    al = rb"16-byte aligned"
    for i in range(2):
        a = [P] * 4
        a[i] += 4
        cases.append((lambda a=a: lib.nd_l2_random_start(*a, 2, 8, 1, 0, 0, 1.0, 0.0, 1.0, None), rb"l2 random start needs " + al))
    for i in range(3):
        a = [P] * 3
        a[i] += 4
        cases.append((lambda a=a: lib.nd_cw_attack_space(*a, 8, 0.0, 1.0, None), rb"cw attack space needs " + al))
    for i in range(6):
        a = [P] * 9
        a[i] += 4
        cases.append((lambda a=a: lib.nd_cw_model_space(*a, 2, 8, 0.0, 1.0, None), rb"cw model space needs " + al))
    for i in range(8):
        a = [P] * 9
        a[i] += 4
        cases.append((lambda a=a: lib.nd_cw_update(*a, 2, 8, 0.01, 0.1, 0.001, 0.5, None), rb"cw update needs " + al))
    assert len(cases) == 16 + 11 + 19
    for call, msg in cases:
        assert call() == -1, msg                                   # ND_ERR_ARG
        assert re.search(msg, lib.nd_last_error()), (msg, lib.nd_last_error())
    # the shape of a row reduction depends on per_image alone
    assert [lib.nd_l2_parts(n) for n in (4, 1024, 1028, 3072, 150528, 4 * 256 * 256, 4 * 256 * 300)] == [1, 1, 2, 3, 147, 256, 256]


class _FakeTensor:
    """What ops' checks ask of a GPU tensor, with no GPU: cw_update hands the fake library nothing but its address."""
    is_cuda, dtype, device = True, torch.float32, "cuda:0"

    def __init__(self, shape):
        self.shape = shape

    def is_contiguous(self):
        return True

    def contiguous(self):
        return self

    def data_ptr(self):
        return 4096


@pytest.mark.parametrize("lo,hi", [(0.0, 1.0), (-1.0, 1.0), (0.25, 0.75), (-0.3, 1.1), (0.1, 0.9)])
def test_cw_update_hands_over_the_b_of_the_model_space_pass(lo, hi, monkeypatch):
    """nd_cw_model_space forms b = (hi - lo) / 2 in float32 from the float32 bounds, and x = t * b + a with it; the tanh-space gradient
    of nd_cw_update must use the same b.  At (-0.3, 1.1) that is 0.70000005 where the double's rounding is 0.7; at (0.1, 0.9) it is
    0.39999998 against 0.4."""
    import ctypes
    import numpy as np
    from nested_diffusion_amd import _lib, ops
    seen = []

    def nd_cw_update(*args):
        seen.append(args)
        return 0

    monkeypatch.setattr(_lib, "load", lambda: types.SimpleNamespace(nd_cw_update=nd_cw_update))
    monkeypatch.setattr(ops.attack_l2, "_stream", lambda t: None)
    shape = (2, 8)
    s = types.SimpleNamespace(B=2, per=8, **{n: _FakeTensor(shape) for n in ("delta", "m", "v", "x", "t", "best")}, flags=_FakeTensor((2,)))
    ops.cw_update(s, _FakeTensor(shape), _FakeTensor(shape), 0.01, 3, lo, hi)
    (args,) = seen
    assert len(args) == len(_lib.SIGNATURES["nd_cw_update"][1]) and args[9:11] == (2, 8)
    want = (np.float32(hi) - np.float32(lo)) / np.float32(2.0)      # the kernel launch's expression: (hi - lo) / 2.0f on float arguments
    assert ctypes.c_float(args[14]).value == float(want), (args[14], want)
    assert args[14] == float(want)                                  # and exactly a float32 already: the ABI's conversion rounds nothing
    if (lo, hi) == (-0.3, 1.1):
        assert float(want) != float(np.float32((hi - lo) / 2.0))    # the case the double's rounding gets wrong


def test_make_attacks_parser_accepts_the_l2_family():
    from nested_diffusion_amd import make_attacks
    for name in ("BIM", "L2PGD"):
        a = make_attacks.build_parser().parse_args(["--config", "c.yml", "--attack_name", name, "--eps", "0.5", "--out", "o"])
        assert a.attack_name == name and a.eps == 0.5
    assert callable(make_attacks.write_attacked_set)


def test_apply_attack_dispatches_to_generate_attack():
    from nested_diffusion_amd import attack
    seen = {}

    class Fake:
        attack_type = "CW"

        def generate_attack(self, samples, labels, first_image=0):
            seen.update(samples=samples, labels=labels, first_image=first_image)
            samples += 1.0                                          # a clone: the caller's tensor must not change
            return samples, torch.ones(len(labels), dtype=torch.bool)

    x, y = torch.zeros(2, 3, 4, 4), torch.tensor([0, 1])
    for name in ("CW", "BIM", "L2PGD"):
        adv = attack.apply_attack(Fake(), x, y, name, first_image=7)
        assert seen["first_image"] == 7 and torch.equal(adv, torch.ones_like(x))
        assert torch.equal(x, torch.zeros_like(x)) and seen["samples"] is not x and seen["labels"] is not y
        assert torch.equal(seen["labels"], y)
