"""Host-side pieces of APGD-L2 and the EOT target (csrc/nd_apgd_l2.hip, autoattack.APGDAttack(norm='L2'), eot.EOTTarget, make_attacks
APGDL2 / --eot): the C ABI, the refusals before any HIP call, the float32 host restatement of the L2 step (which tests/test_gpu_apgd_l2.py
compares the GPU against), the attack's attributes and the parser (no GPU needed)."""
import os
import re
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = types.SimpleNamespace(device="cpu")
F32 = np.float32
INF = float("inf")
ENTRY_POINTS = {"nd_apgd_l2_random_start": 13, "nd_apgd_l2_step": 14, "nd_eot_add": 5}
APGD_L2_START_TAG = 0x41504C32
APGD_RESTORE = 4


# ---- the float32 host restatement of nd_apgd_l2_step (the listing of include/nested_diffusion.h), shared with the GPU tests ---------------
def norm64(v):
    """[B] float32: sqrt of the float64 sum of squares of the fp32 rows of v, rounded once."""
    return np.sqrt((v.astype(np.float64) ** 2).sum(axis=1)).astype(F32)


def project32(x, d, n, eps):
    """clip(x + (d / (n + 1e-12)) * min(eps, n), 0, 1), every operation one fp32 rounding; n [B]."""
    den, m = (n + F32(1e-12)).reshape(-1, 1), np.minimum(F32(eps), n).reshape(-1, 1)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.clip(x + (d / den) * m, F32(0.0), F32(1.0))


def l2_step32(x, xa, xold, g, s, eps, a, norms=None):
    """One L2 momentum step on [B, per] float32 rows: (x_adv, x_adv_old, norms [3, B], (d1, d2)).  g: the row's gradient (the caller
    picks grad_best for a restored row), s [B] the step sizes.  norms None: the norms are computed in float64 and rounded; else the
    given (gn, n1, n2) are used, as the GPU's elementwise passes use theirs."""
    a, one_minus_a = F32(a), F32(1.0) - F32(a)
    gn = norm64(g) if norms is None else norms[0]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        u = xa + s.reshape(-1, 1) * (g / (gn + F32(1e-12)).reshape(-1, 1))
    u = np.where((gn < F32(INF)).reshape(-1, 1), u, xa)          # a NaN or infinite gradient norm: no gradient step
    d1 = u - x
    n1 = norm64(d1) if norms is None else norms[1]
    z = project32(x, d1, n1, eps)
    v = (xa + (z - xa) * a) + (xa - xold) * one_minus_a
    d2 = v - x
    n2 = norm64(d2) if norms is None else norms[2]
    return project32(x, d2, n2, eps), xa.copy(), np.stack([gn, n1, n2]), (d1, d2)


# ---- 1. ABI -----------------------------------------------------------------------------------------------------------------------------
def test_header_signatures_sources_and_library_carry_the_entry_points():
    from nested_diffusion_amd import _lib, build, ops
    with open(os.path.join(ROOT, "include", "nested_diffusion.h")) as f:
        hdr = f.read()
    for name, n_args in ENTRY_POINTS.items():
        assert re.search(rf"\bint {name}\(", hdr), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args, name
        assert hasattr(ops, name[3:]), name
    assert "nd_apgd_l2.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "nd_apgd_l2.hip"))
    tags = {n: int(v, 16) for n, v in re.findall(r"#define (ND_\w+_TAG) (0x[0-9A-Fa-f]+)u", hdr)}
    assert tags["ND_APGD_L2_START_TAG"] == APGD_L2_START_TAG
    for other in ("ND_APGD_START_TAG", "ND_L2_START_TAG", "ND_LINF_START_TAG", "ND_SQUARE_INIT_TAG", "ND_SQUARE_STEP_TAG"):
        assert tags[other] != tags["ND_APGD_L2_START_TAG"], other
    assert len(set(tags.values())) == len(tags)
    assert ops.APGD_RESTORE == APGD_RESTORE
    # the row sum has one copy, which both L2 units include
    with open(os.path.join(build.CSRC, "nd_attack_l2.hip")) as f:
        assert "float l2_block_sum(" not in f.read()
    with open(os.path.join(build.CSRC, "nd_attack.hpp")) as f:
        assert "float l2_block_sum(" in f.read()
    build.build()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name


# ---- 2. refusals before any HIP call ----------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_before_any_hip_call():
    from nested_diffusion_amd import _lib, build
    build.build()
    lib = _lib.load()
    P = 4096                                                       # a dummy non-NULL, 16-byte aligned address, never dereferenced
    start = lambda x0=P, out=P, B=2, per=8: lib.nd_apgd_l2_random_start(x0, P, out, P, P, B, per, 1, 0, 0.5, 0.0, 1.0, None)   # noqa: E731
    step = lambda x=P, B=2, per=8, flags=None, gb=None, xa=P: lib.nd_apgd_l2_step(x, xa, P, P, gb, flags, P, P, P, B, per, 0.5, 0.75, None)   # noqa: E731
    cases = [
        (lambda: start(B=0), rb"nd_apgd_l2_random_start needs 1 <= B <= 65535"),
        (lambda: start(B=65536), rb"nd_apgd_l2_random_start needs 1 <= B <= 65535"),
        (lambda: start(per=6), rb"nd_apgd_l2_random_start.*per_image % 4 == 0"),
        (lambda: start(x0=None), rb"nd_apgd_l2_random_start: NULL"),
        (lambda: start(out=None), rb"nd_apgd_l2_random_start: NULL"),
        (lambda: start(x0=P + 4), rb"nd_apgd_l2_random_start needs 16-byte aligned"),
        (lambda: step(B=0), rb"nd_apgd_l2_step needs 1 <= B <= 65535"),
        (lambda: step(per=10), rb"nd_apgd_l2_step.*per_image % 4 == 0"),
        (lambda: step(x=None), rb"nd_apgd_l2_step: NULL"),
        (lambda: step(xa=None), rb"nd_apgd_l2_step: NULL"),
        (lambda: step(flags=P), rb"nd_apgd_l2_step with flags needs grad_best"),
        (lambda: step(x=P + 8), rb"nd_apgd_l2_step needs 16-byte aligned"),
        (lambda: lib.nd_eot_add(None, P, 8, 0, None), rb"nd_eot_add: NULL"),
        (lambda: lib.nd_eot_add(P, None, 8, 0, None), rb"nd_eot_add: NULL"),
        (lambda: lib.nd_eot_add(P, P, 6, 0, None), rb"nd_eot_add needs n % 4 == 0"),
        (lambda: lib.nd_eot_add(P, P, 8, -1, None), rb"nd_eot_add needs .*divisor >= 0"),
        (lambda: lib.nd_eot_add(P + 4, P, 8, 2, None), rb"nd_eot_add needs 16-byte aligned"),
    ]
    for call, msg in cases:
        assert call() == -1, msg                                   # ND_ERR_ARG
        assert re.search(msg, lib.nd_last_error()), (msg, lib.nd_last_error())


# ---- 3. the listing itself ------------------------------------------------------------------------------------------------------------------
LISTING = ("g2 = xa - x_adv_old;  x_adv_old = xa",
           "gn = n(g);            u  = xa + s * (g / (gn + 1e-12))",
           "d1 = u - x;  n1 = n(d1);  z = clip(x + (d1 / (n1 + 1e-12)) * min(eps, n1), 0, 1)",
           "v  = (xa + (z - xa) * a) + g2 * (1 - a)",
           "d2 = v - x;  n2 = n(d2);  x_adv = clip(x + (d2 / (n2 + 1e-12)) * min(eps, n2), 0, 1)")


def header_listing():
    """The five lines of nd_apgd_l2_step's listing in the header, which l2_step32 restates line for line."""
    with open(os.path.join(ROOT, "include", "nested_diffusion.h")) as f:
        hdr = f.read()
    sec = hdr[hdr.index("nd_apgd_l2_step "):hdr.index("#define ND_APGD_L2_START_TAG")]
    lines = [line.strip(" *") for line in sec.splitlines()]
    assert [line for line in lines if line in LISTING] == list(LISTING)
    return LISTING


@pytest.mark.parametrize("a", [1.0, 0.75])
@pytest.mark.parametrize("per", [4, 3072])
def test_host_listing_stays_in_the_ball_and_the_box(per, a):
    assert len(header_listing()) == 5                            # what is checked below is the header's listing
    B, eps = 6, 0.5
    rng = np.random.default_rng(1000 + per)
    x = rng.random((B, per), dtype=F32)
    for trial in range(8):
        # iterates anywhere in the box (the momentum term may come from outside the ball), gradients of differing magnitude
        xa = np.clip(x + F32(0.3) * rng.standard_normal((B, per), dtype=F32), F32(0), F32(1))
        xold = xa.copy() if a == 1.0 else np.clip(x + F32(0.3) * rng.standard_normal((B, per), dtype=F32), F32(0), F32(1))
        g = rng.standard_normal((B, per), dtype=F32) * (F32(10.0) ** np.arange(-3, B - 3, dtype=F32)).reshape(B, 1)
        s = np.full(B, 2 * eps, F32) / F32(2.0) ** rng.integers(0, 4, B).astype(F32)
        out, old, norms, _ = l2_step32(x, xa, xold, g, s, eps, a)
        assert np.array_equal(old, xa) and np.isfinite(norms).all()
        assert out.min() >= 0.0 and out.max() <= 1.0
        dist = np.sqrt(((out.astype(np.float64) - x.astype(np.float64)) ** 2).sum(axis=1))
        assert (dist <= eps * (1 + per * 2.0 ** -24)).all(), (trial, dist.max())


def test_host_listing_skips_the_gradient_step_of_a_nan_row():
    with open(os.path.join(ROOT, "include", "nested_diffusion.h")) as f:
        assert "A row whose gn is NaN\n" in f.read().split("nd_apgd_l2_step ")[1]       # the documented deviation this restates
    rng = np.random.default_rng(5)
    x = rng.random((2, 8), dtype=F32)
    xa = np.clip(x + F32(0.01), F32(0), F32(1))
    g = rng.standard_normal((2, 8), dtype=F32)
    g[1, 3] = np.nan
    norms = np.stack([np.array([norm64(g[:1])[0], np.nan], F32), np.zeros(2, F32), np.zeros(2, F32)])
    out, _, used, (d1, _) = l2_step32(x, xa, xa.copy(), g, np.full(2, 0.1, F32), 100.0, 1.0)
    assert np.isnan(used[0, 1]) and np.isfinite(out).all()
    assert np.array_equal(d1[1], xa[1] - x[1]) and not np.array_equal(d1[0], xa[0] - x[0])
    assert norms.shape == used.shape


# ---- 4. APGDAttack(norm='L2') ---------------------------------------------------------------------------------------------------------------
def test_apgd_l2_attributes_and_the_refusals_that_stay():
    from nested_diffusion_amd.autoattack import APGDAttack
    p = APGDAttack(FAKE, norm="L2", eps=0.5)
    q = APGDAttack(FAKE, eps=0.5)
    assert p.norm == "L2" and q.norm == "Linf"
    assert p.schedule == q.schedule and sorted(p.schedule) == [21, 40, 56, 69, 79, 86, 92, 98]
    assert (p.n_iter, p.n_restarts, p.n_iter_2, p.n_iter_min, p.size_decr, p.thr_decr) == (100, 1, 22, 6, 3, 0.75)
    assert p.attack_type == "APGD" and APGDAttack.attack_type == "APGD"
    assert p.epsilon == 0.5 and p.eps == 0.5
    p.eps = 0.25
    assert p.epsilon == 0.25                                       # one value under two names
    assert callable(p.generate_attack)
    for kwargs, match in ((dict(norm="L1"), "L1"), (dict(loss="dlr"), "dlr"), (dict(eot_iter=2), "eot_iter")):
        with pytest.raises(NotImplementedError, match=match):
            APGDAttack(FAKE, eps=0.1, **kwargs)
        with pytest.raises(NotImplementedError, match=match):
            APGDAttack(FAKE, eps=0.1, **{"norm": "L2", **kwargs})


# ---- 5. EOTTarget ------------------------------------------------------------------------------------------------------------------------------
class FakeModel:
    device = "cpu"

    def __init__(self):
        self.calls, self.out = 0, (object(), object(), object())

    def forward(self, x):
        return ("forward", x)

    def input_grad(self, x, labels):
        self.calls += 1
        return self.out


def test_eot_target_refusals_passthrough_and_surface():
    from nested_diffusion_amd import attack
    from nested_diffusion_amd.eot import EOTTarget
    m = FakeModel()
    for bad in (0, -3):
        with pytest.raises(ValueError, match="at least one draw"):
            EOTTarget(m, bad)
    for bad in (1.5, 2.0, "2", None, True):
        with pytest.raises(TypeError, match="integer"):
            EOTTarget(m, bad)
    with pytest.raises(TypeError, match="input_grad"):
        EOTTarget(types.SimpleNamespace(device="cpu", forward=lambda x: x), 2)
    assert m.calls == 0                                            # refused before anything runs
    t = EOTTarget(m, 1)
    assert not hasattr(t, "vit") and attack._vit(t) is t
    assert t.device == "cpu" and t.n == 1 and t.model is m
    out = t.input_grad("x", "y")
    assert out is m.out and m.calls == 1                           # n = 1: the wrapped result itself, one call
    assert t.forward("x") == ("forward", "x") and t("x") == ("forward", "x")
    with pytest.raises(NotImplementedError, match="EOTTarget"):
        t.input_grad_margin("x", "y", None)
    with pytest.raises(NotImplementedError, match="EOTTarget"):
        EOTTarget(m, 4).input_grad_margin()
    # a wrapped GuidingConditioner-like object is not unwrapped either
    assert attack._vit(EOTTarget(types.SimpleNamespace(device="cpu", vit=FAKE, input_grad=lambda x, y: None), 2)).n == 2


# ---- 6. make_attacks ------------------------------------------------------------------------------------------------------------------------------
def test_make_attacks_parser_apgdl2_and_eot(tmp_path):
    from nested_diffusion_amd import make_attacks
    from nested_diffusion_amd.autoattack import APGDAttack
    from nested_diffusion_amd.eot import EOTTarget
    base = ["--config", str(tmp_path / "missing.yml"), "--eps", "0.5", "--out", "o"]
    a = make_attacks.build_parser().parse_args(base + ["--attack_name", "APGDL2"])
    assert a.attack_name == "APGDL2" and not hasattr(a, "eot")
    b = make_attacks.build_parser().parse_args(base + ["--attack_name", "PGD"])
    assert vars(b) == {**vars(a), "attack_name": "PGD"}            # no new key in a run without the new flags
    m = FakeModel()
    assert make_attacks.eot_wrap(a, m) is m                        # without --eot no wrapper is built
    atk = make_attacks.make_named_attack(a, m)
    assert isinstance(atk, APGDAttack) and (atk.norm, atk.eps, atk.n_restarts, atk.n_iter, atk.seed) == ("L2", 0.5, 5, 100, 0)
    assert atk.model is m
    e = make_attacks.build_parser().parse_args(base + ["--attack_name", "APGDL2", "--eot", "3", "--seed", "4"])
    w = make_attacks.eot_wrap(e, m)
    assert isinstance(w, EOTTarget) and w.n == 3 and w.model is m
    assert make_attacks.make_named_attack(e, w).model is w and make_attacks.make_named_attack(e, w).seed == 4
    for n in ("0", "-2"):                                          # refused before the (missing) config is opened or the GPU touched
        with pytest.raises(SystemExit, match="--eot must be at least 1"):
            make_attacks.main(base + ["--attack_name", "APGDL2", "--eot", n])
    with pytest.raises(SystemExit):
        make_attacks.build_parser().parse_args(base + ["--attack_name", "APGDL2", "--eot", "1.5"])
    with pytest.raises(FileNotFoundError):                         # a valid --eot gets as far as the config
        make_attacks.main(base + ["--attack_name", "APGDL2", "--eot", "2"])
