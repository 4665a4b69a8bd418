"""The EMA shadow of the noise estimators, host side (no GPU): the float32 listing of nd_clip_adam_ema's shadow update against the
reference's EMA class (tests/golden/ema.npz, written by tests/golden/gen_ema_golden.py from diffusion/ema.py), the coefficients of
ops.ema_step, the refusals of the entry point (all before any launch), the flags, and the snapshot / checkpoint refusals by name.
ema_f32 is what tests/test_gpu_ema.py holds the kernel to."""
import argparse
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ND_ERR_ARG = -1                                            # include/nested_diffusion.h


def ema_f32(w_new, s, mu):
    """nd_clip_adam_ema's three operations on the weight the optimizer wrote: each coefficient rounded ONCE from double, two rounded
    products, one rounded sum (numpy's float32 arithmetic neither contracts nor flushes denormals)."""
    c1, c2 = np.float32(1.0 - float(mu)), np.float32(float(mu))
    with np.errstate(all="ignore"):
        pw = c1 * np.asarray(w_new, dtype=np.float32)
        ps = c2 * np.asarray(s, dtype=np.float32)
        return pw + ps


def ema_wrong_one_minus_mu(w_new, s, mu):
    """the first mistake: 1 - mu formed in float32"""
    c2 = np.float32(float(mu))
    c1 = np.float32(1.0) - c2
    with np.errstate(all="ignore"):
        return c1 * np.asarray(w_new, dtype=np.float32) + c2 * np.asarray(s, dtype=np.float32)


def ema_contracted(w_new, s, mu, which=0):
    """the second mistake: one product kept unrounded inside a fused multiply-add (float64 holds a product of two float32 exactly, and
    the sum of it and a float32, rounded to float32 once, is the fma wherever the float64 sum is itself exact or far from a tie; the
    test below only needs it to DIFFER somewhere).  which: the product that stays unrounded."""
    c1, c2 = np.float32(1.0 - float(mu)), np.float32(float(mu))
    w_new, s = np.asarray(w_new, dtype=np.float32), np.asarray(s, dtype=np.float32)
    with np.errstate(all="ignore"):
        if which == 0:
            return (np.float64(c1) * w_new.astype(np.float64) + (c2 * s).astype(np.float64)).astype(np.float32)
        return ((c1 * w_new).astype(np.float64) + np.float64(c2) * s.astype(np.float64)).astype(np.float32)


def same_bits(a, b):
    """bit equality of two float32 arrays; a NaN must face a NaN (its payload is not compared)"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]))


def differing(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    both = ~(np.isnan(a) | np.isnan(b))
    return int((a.view(np.uint32)[both] != b.view(np.uint32)[both]).sum())


@pytest.fixture(scope="module")
def fixture():
    z = np.load(os.path.join(GOLDEN, "ema.npz"))
    return {k: z[k] for k in z.files}


# ---- 1. the listing against the reference's EMA class ------------------------------------------------------------------------------------
def walk(form, params, mu):
    """the shadow after each update, CHAINED from register(): an error at one update is carried into every later one"""
    s, out = params[0].copy(), []
    for u in range(1, params.shape[0]):
        s = form(params[u], s, mu)
        out.append(s)
    return np.stack(out)


def test_fixture_holds_what_the_issue_asks_for(fixture):
    rates, params, shadow = fixture["rates"], fixture["params"], fixture["shadow"]
    assert list(rates) == [0.9999, 0.5] and rates.dtype == np.float64
    U = params.shape[0] - 1
    assert U >= 8 and shadow.shape == (2, U, params.shape[1]) and params.dtype == shadow.dtype == np.float32
    assert os.path.getsize(os.path.join(GOLDEN, "ema.npz")) < 64 * 1024
    p = params
    tiny = np.finfo(np.float32).tiny
    assert np.isnan(p).any() and np.isposinf(p).any() and np.isneginf(p).any()
    assert ((p == 0) & ~np.signbit(p)).any() and ((p == 0) & np.signbit(p)).any()
    assert (p == np.float32(1e-40)).any() and (p == np.finfo(np.float32).max).any()
    prod = np.float32(1.0 - 0.9999) * p[np.isfinite(p)]
    assert ((np.abs(p[np.isfinite(p)]) >= tiny) & (prod != 0) & (np.abs(prod) < tiny)).any()      # normal, its product with 1e-4 denormal
    assert np.isfinite(p).sum() >= 3000
    # the shadow itself meets denormals, infinities and NaN
    assert np.isnan(shadow).any() and np.isinf(shadow).any() and ((shadow != 0) & (np.abs(shadow) < tiny)).any()


def test_listing_reproduces_the_reference_bit_for_bit(fixture):
    for r, mu in enumerate(fixture["rates"]):
        got = walk(ema_f32, fixture["params"], mu)
        for u in range(got.shape[0]):
            assert same_bits(got[u], fixture["shadow"][r, u]), (mu, u, differing(got[u], fixture["shadow"][r, u]))


def test_each_wrong_form_differs_from_the_reference_somewhere(fixture):
    params, shadow = fixture["params"], fixture["shadow"][0]                   # mu = 0.9999 (at 0.5 both products are exact)
    n_c1 = differing(walk(ema_wrong_one_minus_mu, params, 0.9999), shadow)
    n_f0 = differing(walk(lambda w, s, mu: ema_contracted(w, s, mu, 0), params, 0.9999), shadow)
    n_f1 = differing(walk(lambda w, s, mu: ema_contracted(w, s, mu, 1), params, 0.9999), shadow)
    print(f"  elements that differ from the reference: float32 1 - mu {n_c1}, contracted (1 - mu) * w {n_f0}, contracted mu * s {n_f1}")
    assert n_c1 > 0 and n_f0 > 0 and n_f1 > 0
    # and in a SINGLE update from the reference's own previous shadow (no accumulated error to lean on)
    prev = np.concatenate([params[:1], shadow[:-1]])
    for form in (ema_wrong_one_minus_mu, lambda w, s, mu: ema_contracted(w, s, mu, 0), lambda w, s, mu: ema_contracted(w, s, mu, 1)):
        assert sum(differing(form(params[u + 1], prev[u], 0.9999), shadow[u]) for u in range(shadow.shape[0])) > 0


@pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="needs the reference checkout the fixture was made from")
def test_generator_check_passes_beside_the_reference():
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "gen_ema_golden.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


# ---- 2. ops.ema_step ------------------------------------------------------------------------------------------------------------------------
def test_ema_step_rounds_each_coefficient_once_from_double():
    from nested_diffusion_amd import _lib, ops
    e = ops.ema_step(0.9999)
    assert isinstance(e, _lib.NdEmaStep)
    assert np.float32(e.one_minus_mu).view(np.uint32) == np.float32(1.0 - 0.9999).view(np.uint32)
    assert np.float32(e.mu).view(np.uint32) == np.float32(0.9999).view(np.uint32)
    assert np.float32(e.one_minus_mu) == np.float32(1e-4) and np.float32(e.one_minus_mu) != np.float32(1.0) - np.float32(0.9999)
    assert ctypes.sizeof(e) == 8


@pytest.mark.parametrize("mu", [0, 1, -0.1, 1.5, float("nan"), float("inf")])
def test_ema_step_refuses_a_rate_outside_the_open_interval(mu):
    from nested_diffusion_amd import ops
    with pytest.raises(ValueError, match="0 < mu < 1"):
        ops.ema_step(mu)


# ---- 3. the entry point's refusals: no device, no launch ---------------------------------------------------------------------------------------
def test_library_exports_and_refuses_before_any_launch():
    from nested_diffusion_amd import _lib, ops
    lib = _lib.load()
    assert hasattr(lib, "nd_clip_adam_ema") and "nd_clip_adam_ema" in _lib.SIGNATURES
    a, e = ops.adam_step(1e-3, 1), ops.ema_step(0.9999)
    A, E = ctypes.byref(a), ctypes.byref(e)
    w, m, v, g, s = (0x1000 * (i + 1) for i in range(5))          # aligned addresses that are never dereferenced: every call is refused
    cases = {"NULL s": ((w, m, v, g, None, 8, None, 1.0, A, E, None), "NULL shadow"),
             "NULL e": ((w, m, v, g, s, 8, None, 1.0, A, None, None), "NULL nd_ema_step"),
             "NULL w": ((None, m, v, g, s, 8, None, 1.0, A, E, None), "NULL tensor"),
             "n = 0": ((w, m, v, g, s, 0, None, 1.0, A, E, None), "n >= 1"),
             "misaligned s": ((w, m, v, g, s + 2, 8, None, 1.0, A, E, None), "misaligned"),
             "misaligned w": ((w + 1, m, v, g, s, 8, None, 1.0, A, E, None), "misaligned"),
             "s == w": ((w, m, v, g, w, 8, None, 1.0, A, E, None), "distinct"),
             "s == g": ((w, m, v, g, g, 8, None, 1.0, A, E, None), "distinct"),
             "m == v": ((w, m, m, g, s, 8, None, 1.0, A, E, None), "distinct")}
    for name, (args, text) in cases.items():
        rc = lib.nd_clip_adam_ema(*args)
        msg = lib.nd_last_error().decode()
        assert rc == ND_ERR_ARG, name
        assert "clip_adam_ema" in msg and text in msg, (name, msg)
    # nd_clip_adam's own refusals keep their words
    assert lib.nd_clip_adam(w, m, v, w, 8, None, 1.0, A, None) == ND_ERR_ARG
    assert "clip_adam: w, m, v and g must be distinct buffers" in lib.nd_last_error().decode()


def test_clip_adam_refuses_half_a_pair_before_it_looks_at_a_tensor():
    from nested_diffusion_amd import ops
    a = ops.adam_step(1e-3, 1)
    t = torch.zeros(4)
    with pytest.raises(ValueError, match="shadow and ema come together"):
        ops.clip_adam(t, t, t, t, a, shadow=t)
    with pytest.raises(ValueError, match="shadow and ema come together"):
        ops.clip_adam(t, t, t, t, a, ema=ops.ema_step(0.5))
    with pytest.raises(TypeError, match="ops.ema_step"):
        ops.clip_adam(t, t, t, t, a, shadow=t, ema=0.5)


# ---- 4. the flags ----------------------------------------------------------------------------------------------------------------------------
def test_main_parser_leaves_no_attribute_without_the_flags():
    from nested_diffusion_amd import main as nd_main
    base = "--config c --doc d --preprocess grayscaled".split()
    ns = nd_main.build_parser().parse_args(base)
    assert "ema" not in vars(ns) and "use_ema" not in vars(ns)
    ns = nd_main.build_parser().parse_args(base + ["--ema"])
    assert ns.ema is True and "use_ema" not in vars(ns)
    ns = nd_main.build_parser().parse_args(base + ["--use_ema", "--test"])
    assert ns.use_ema is True and "ema" not in vars(ns)


def test_train_refuses_a_missing_or_impossible_rate_by_name_before_anything_is_built(tmp_path):
    from nested_diffusion_amd.runner import Diffusion
    ns = argparse.Namespace
    for model in (ns(), ns(ema_rate=1.0), ns(ema_rate=0.0), ns(ema_rate=float("nan")), ns(ema_rate="0.9"), ns(ema_rate=True)):
        runner = object.__new__(Diffusion)
        runner.args = ns(log_path=str(tmp_path), ema=True)
        runner.config = ns(diffusion=ns(aux_cls=ns(arch="sevit")), model=model)
        runner.cond_pred_model = ns(mlps=[None, None])
        runner.operand_dtype = "f32"
        with pytest.raises(ValueError, match="model.ema_rate"):
            runner.train(0, train_loader=[], valid_loader=[])


# ---- 5. snapshots and checkpoints refuse by name ---------------------------------------------------------------------------------------------
def test_check_meta_names_ema_rate_in_every_mismatch():
    from nested_diffusion_amd import snapshot
    base = {"format": snapshot.FORMAT, "kind": "noise_estimator", "num_classes": 2}
    with_ema = dict(base, ema_rate=0.9999)
    snapshot.check_meta(base, base)
    snapshot.check_meta(with_ema, with_ema)
    with pytest.raises(ValueError, match=r"^ema_rate: the snapshot does not record it"):            # a run with EMA, a snapshot without
        snapshot.check_meta(base, with_ema)
    with pytest.raises(ValueError, match=r"^ema_rate: .*this run has none"):                        # a run without, a snapshot with
        snapshot.check_meta(with_ema, base)
    with pytest.raises(ValueError, match=r"^ema_rate: .*0\.9999.*0\.999\b"):                        # another rate
        snapshot.check_meta(with_ema, dict(base, ema_rate=0.999))


def test_use_ema_reader_names_the_checkpoint_without_an_ema_entry(tmp_path):
    from nested_diffusion_amd.runner import Diffusion
    ns = argparse.Namespace
    sd, sd_ema = {"lin4.bias": torch.zeros(2)}, {"lin4.bias": torch.ones(2)}
    plain, both = str(tmp_path / "plain.pth"), str(tmp_path / "both.pth")
    torch.save({"noise_estimator": sd, "optimizer": {"step": 1, "lr": 1e-3}, "epoch": 0}, plain)
    torch.save({"noise_estimator": sd, "optimizer": {"step": 1, "lr": 1e-3}, "epoch": 0, "ema": sd_ema}, both)

    def reader(paths, **flags):
        runner = object.__new__(Diffusion)
        runner.args = ns(**flags)
        runner.config = ns(diffusion=ns(trained_diffusion_ckpt_path=[paths]))
        runner.num_noise_estimators_required = 6
        return runner._read_noise_estimator_states()

    assert float(reader([both, plain])[0]["lin4.bias"][0]) == 0.0                                  # no flag: the live weights, as always
    assert float(reader([both], use_ema=False)[0]["lin4.bias"][0]) == 0.0
    assert float(reader([both], use_ema=True)[0]["lin4.bias"][0]) == 1.0
    with pytest.raises(KeyError) as err:
        reader([both, plain], use_ema=True)
    assert plain in str(err.value) and "--use_ema" in str(err.value) and "'ema'" in str(err.value)
