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


@pytest.mark.parametrize("rho", [0.75, 0.5])
def test_apgd_restatements_agree_bit_for_bit_on_a_synthetic_run(rho):
    """The oracle of tests/test_gpu_apgd_edges.py checked where no GPU is needed: ref_control and ref_update (per-kernel, numpy, a literal
    transcription of the listing) against HostAPGD (whole-array torch, in autopgd_base.py's style, written independently) over one random
    synthetic run of the production schedule: every state array, every iteration, bit for bit."""
    import numpy as np
    from nested_diffusion_amd.autoattack import apgd_schedule
    from test_gpu_apgd import HostAPGD
    from test_gpu_apgd_edges import ref_control, ref_new_state, ref_update, same
    B, C, n_iter, eps, shape = 384, 3, 100, 8 / 255, (3, 2, 2)
    per = int(np.prod(shape))
    schedule = apgd_schedule(n_iter, 22, 6, 3)
    assert len(schedule) == 8
    rng = np.random.default_rng(77)
    f32 = np.float32

    level, rise = np.zeros(B, f32), np.linspace(0.0, 1.0, B)

    def draw():
        logits = rng.standard_normal((B, C)).astype(f32)
        grad = rng.standard_normal((B, per)).astype(f32)
        grad[rng.random((B, per)) < 0.05] = 0.0
        grad[rng.random((B, per)) < 0.02] = np.nan
        grad[rng.random((B, per)) < 0.02] = np.inf
        level[:] = level + np.where(rng.random(B) < rise, f32(0.25), f32(-0.25)) * (rng.random(B) < 0.9).astype(f32)
        loss = level.copy()                                        # a walk per row that rises with the row's own probability, with ties
        loss[rng.random(B) < 0.01] = np.nan
        loss[rng.random(B) < 0.01] = np.inf
        return logits, grad, loss

    x = rng.random((B, per), dtype=f32)
    x[rng.random((B, per)) < 0.1] = 0.0
    x[rng.random((B, per)) < 0.1] = 1.0
    x_adv = np.clip(x + f32(eps) * (f32(2.0) * rng.random((B, per), dtype=f32) - f32(1.0)), f32(0.0), f32(1.0))
    y = rng.integers(0, C, B)
    t4 = lambda a: torch.from_numpy(a.copy()).reshape(B, *shape)                                   # noqa: E731
    logits, grad, loss = draw()
    host = HostAPGD(t4(x), torch.from_numpy(y), eps, n_iter, schedule, rho=rho)
    host.init(t4(x_adv), torch.from_numpy(logits), t4(grad), torch.from_numpy(loss))
    host.do_step(0)
    st = ref_new_state(B, n_iter)
    ref_control(st, logits, y, loss, -1, 0, rho, step0=2.0 * eps)
    a = dict(x=x, x_adv=x_adv, x_adv_old=x_adv.copy(), grad=grad, x_best=x_adv.copy(), grad_best=grad.copy(), x_best_adv=x_adv.copy())
    ref_update(a, None, st["step"], eps, 1.0, True)

    def compare(where):
        for n in ("x_adv", "x_adv_old", "x_best", "grad_best", "x_best_adv"):
            same(n, getattr(host, n).reshape(B, per), a[n], where)
        for n in ("step", "loss_best", "loss_best_last_check", "loss_steps"):
            same(n, getattr(host, n), st[n], where)
        same("reduced_last_check", host.reduced_last_check.to(torch.int32), st["reduced_last_check"], where)
        same("acc", host.acc.to(torch.int32), st["acc"], where)

    compare("after the first step")
    seen = set()
    for i in range(n_iter):
        logits, grad, loss = draw()
        host.observe(i, torch.from_numpy(logits), t4(grad), torch.from_numpy(loss))
        if i + 1 < n_iter:
            host.do_step(i + 1)
        a["grad"] = grad
        ref_control(st, logits, y, loss, i, schedule.get(i, 0), rho)
        ref_update(a, st["flags"], st["step"], eps, 0.75, i + 1 < n_iter)
        compare(f"after iteration {i}")
        seen |= set(int(v) for v in st["flags"])
    assert seen == set(range(8))                                   # the run passed every flag value from control to update
    assert host.restores >= B and host.keeps >= B // 2             # and both outcomes of the checkpoint rule, many times
    assert len(set(st["step"].tolist())) >= 4
