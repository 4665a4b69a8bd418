"""Host-side pieces of AutoAttack's APGD-CE (nested_diffusion_amd/autoattack.py): constructor constants, the checkpoint schedule, the
refusals, apply_attack's AUTOPGD dispatch, make_attacks' parser and the C ABI declarations of the APGD kernels (no GPU needed)."""
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APGD_SYMBOLS = ["nd_apgd_random_start", "nd_apgd_control", "nd_apgd_update"]
FAKE = types.SimpleNamespace(device="cpu")


def test_autoattack_constructor_matches_the_reference_call():
    from nested_diffusion_amd.autoattack import AutoAttack
    a = AutoAttack(FAKE, eps=8 / 255, version="custom", norm="Linf", attacks_to_run=["apgd-ce"])
    assert a.attack_type == "AUTOPGD"
    assert (a.norm, a.epsilon, a.seed, a.version, a.attacks_to_run) == ("Linf", 8 / 255, None, "custom", ["apgd-ce"])
    p = a.apgd
    assert (p.n_restarts, p.n_iter, p.eps, p.norm, p.eot_iter, p.thr_decr, p.loss) == (5, 100, 8 / 255, "Linf", 1, 0.75, "ce")
    assert (p.n_iter_2, p.n_iter_min, p.size_decr) == (22, 6, 3)
    assert p.seed == 0 and a.get_seed() == 0                       # seed=None becomes 0
    assert AutoAttack(FAKE, eps=0.1, seed=9, version="custom", attacks_to_run=["apgd-ce"]).apgd.seed == 9
    # a GuidingConditioner is accepted for its ViT
    assert AutoAttack(types.SimpleNamespace(vit=FAKE), eps=0.1, version="custom", attacks_to_run=["apgd-ce"]).model is FAKE


@pytest.mark.parametrize("n_iter,want", [(100, [21, 40, 56, 69, 79, 86, 92, 98]), (30, [5, 10, 14, 17, 19] + list(range(20, 30)))])
def test_checkpoint_schedule(n_iter, want):
    from nested_diffusion_amd.autoattack import APGDAttack
    p = APGDAttack(FAKE, n_iter=n_iter, eps=0.1)
    assert sorted(p.schedule) == want
    ks = [p.schedule[i] for i in want]
    assert ks[0] == p.n_iter_2
    assert all(k == max(prev - p.size_decr, p.n_iter_min) for prev, k in zip(ks, ks[1:]))
    # each checkpoint follows the previous one after k iterations: the oscillation count never reaches past the first row
    assert all(i - j == p.schedule[i] for j, i in zip([-1] + want, want))


@pytest.mark.parametrize("kwargs,match", [
    (dict(version="standard"), r"standard.*apgd-t.*fab-t.*square"),
    (dict(version="plus"), "plus"),
    (dict(version="rand"), "rand"),
    (dict(version="custom", norm="L2", attacks_to_run=["apgd-ce"]), "L2"),
    (dict(version="custom", attacks_to_run=["apgd-ce", "apgd-t"]), "apgd-t"),
    (dict(version="custom", attacks_to_run=["fab"]), "fab"),
    (dict(version="custom", attacks_to_run=["fab-t"]), "fab-t"),
    (dict(version="custom", attacks_to_run=["square"]), "square"),
    (dict(version="custom", attacks_to_run=["apgd-dlr"]), "apgd-dlr"),
])
def test_unbuilt_autoattack_configurations_name_themselves(kwargs, match):
    from nested_diffusion_amd.autoattack import AutoAttack
    with pytest.raises(NotImplementedError, match=match):
        AutoAttack(FAKE, eps=0.1, **kwargs)


def test_apgd_refusals():
    from nested_diffusion_amd.autoattack import APGDAttack
    for kwargs, match in ((dict(norm="L1"), "L1"), (dict(loss="dlr"), "dlr"), (dict(eot_iter=2), "eot_iter")):
        with pytest.raises(NotImplementedError, match=match):
            APGDAttack(FAKE, eps=0.1, **kwargs)


def test_attack_class_still_refuses_autopgd():
    from nested_diffusion_amd import attack
    with pytest.raises(NotImplementedError, match="AUTOPGD"):
        attack.Attack(0.1, "AUTOPGD", FAKE)
    with pytest.raises(NotImplementedError, match="AUTOPGD"):
        attack.apply_attack(types.SimpleNamespace(run_standard_evaluation=lambda *a, **k: None), torch.zeros(1), torch.zeros(1), "AUTOPGD")


def test_apply_attack_dispatches_autopgd_to_run_standard_evaluation():
    from nested_diffusion_amd import attack
    from nested_diffusion_amd.autoattack import AutoAttack
    calls = []

    class Fake(AutoAttack):
        def __init__(self):
            pass

        def run_standard_evaluation(self, x, y, bs=250, first_image=0):
            calls.append((x, y, bs, first_image))
            return x + 1

    x, y = torch.rand(5, 3, 4, 4), torch.tensor([0, 1, 0, 1, 1])
    out = attack.apply_attack(Fake(), x, y, "AUTOPGD", first_image=40)
    (cx, cy, bs, first), = calls
    assert bs == 5 and first == 40                                 # bs = labels.shape[0], as utils.py:263-266
    assert torch.equal(cx, x) and cx is not x and torch.equal(cy, y)   # the inputs are not modified
    assert torch.equal(out, x + 1)


def test_make_attacks_parser_accepts_autopgd():
    from nested_diffusion_amd import make_attacks
    a = make_attacks.build_parser().parse_args(["--config", "c.yml", "--attack_name", "AUTOPGD", "--eps", "0.03", "--out", "o"])
    assert a.attack_name == "AUTOPGD" and a.seed == 0
    with pytest.raises(SystemExit):
        make_attacks.build_parser().parse_args(["--config", "c.yml", "--attack_name", "CW", "--eps", "0.03", "--out", "o"])


def test_header_and_signatures_carry_the_apgd_entry_points():
    from nested_diffusion_amd import _lib, build, ops
    with open(os.path.join(ROOT, "include", "nested_diffusion.h")) as f:
        hdr = f.read()
    for s in APGD_SYMBOLS:
        assert re.search(rf"\bint {s}\(", hdr), s
        assert s in _lib.SIGNATURES, s
        assert hasattr(ops, s[3:]), s
    assert "ND_APGD_START_TAG 0x41504731u" in hdr
    assert "ND_LINF_START_TAG 0x41544B31u" in hdr                  # a tag of its own: APGD and PGD starts are independent draws
    for name, v in (("NOT_PRED", 1), ("IMPROVED", 2), ("RESTORE", 4)):
        assert f"ND_APGD_{name} {v}" in hdr and getattr(ops, f"APGD_{name}") == v
    build.build()
    lib = _lib.load()
    for s in APGD_SYMBOLS:
        assert hasattr(lib, s), s


def test_apgd_kernels_refuse_bad_arguments_before_any_launch():
    from nested_diffusion_amd import _lib, build
    build.build()
    lib = _lib.load()
    P = 4096                                                       # a dummy non-NULL, 16-byte aligned address, never dereferenced
    cases = [
        (lambda: lib.nd_apgd_random_start(P, P, P, P, 2, 6, 1, 0, 0.1, 0.0, 1.0, None), rb"per_image % 4 == 0"),
        (lambda: lib.nd_apgd_random_start(P, P, P, P, 0, 8, 1, 0, 0.1, 0.0, 1.0, None), rb"1 <= B <= 65535"),
        (lambda: lib.nd_apgd_random_start(P + 4, P, P, P, 2, 8, 1, 0, 0.1, 0.0, 1.0, None), rb"16-byte aligned"),
        (lambda: lib.nd_apgd_random_start(P, None, P, P, 2, 8, 1, 0, 0.1, 0.0, 1.0, None), rb"NULL tensor"),
        (lambda: lib.nd_apgd_control(P, P, P, P, P, P, P, P, P, P, 2, 1025, 100, 0, 0, 0.75, 0.0, None), rb"C <= 1024 \(C=1025\)"),
        (lambda: lib.nd_apgd_control(P, P, P, P, P, P, P, P, P, P, 2, 2, 100, 100, 0, 0.75, 0.0, None), rb"iter < n_iter"),
        (lambda: lib.nd_apgd_control(P, P, P, P, P, P, P, P, P, P, 2, 2, 100, 5, 7, 0.75, 0.0, None), rb"k <= iter \+ 1 \(iter=5, k=7"),
        (lambda: lib.nd_apgd_control(P, P, P, P, P, P, P, P, P, None, 2, 2, 100, 5, 0, 0.75, 0.0, None), rb"NULL tensor"),
        (lambda: lib.nd_apgd_update(P, P, P, P, P, P, P, P, P, 2, 6, 0.1, 0.75, 1, None), rb"per_image % 4 == 0"),
        (lambda: lib.nd_apgd_update(P, P, P, P, P, P, P + 8, P, P, 2, 8, 0.1, 0.75, 1, None), rb"16-byte aligned"),
        (lambda: lib.nd_apgd_update(P, P, P, P, None, P, P, P, P, 2, 8, 0.1, 0.75, 1, None), rb"with flags needs"),
        (lambda: lib.nd_apgd_update(P, P, None, P, None, None, None, None, P, 2, 8, 0.1, 1.0, 1, None), rb"with a step needs"),
    ]
    for call, msg in cases:
        assert call() == -1, msg                                   # ND_ERR_ARG
        assert re.search(msg, lib.nd_last_error()), (msg, lib.nd_last_error())
