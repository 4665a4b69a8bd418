"""Host checks of the noise-estimator training step: the autograd oracle (tests/_diffusion_train_oracle.py) against the reference's own
five recorded steps (tests/golden/diffusion_train.npz), the ABI of the new entry points, check_step_args' refusals and the CLI flag.

Bounds.  The fixture is the reference in fp32.  The oracle in fp32 runs the same torch operations (here it agrees bit for bit; another
host's thread count may change torch's summation order), the oracle in fp64 differs from the fixture by the reference's own fp32 error
(measured here: 5.6e-7 on the step-0 gradients, 6e-7 on the losses, 1.7e-5 on the norms, 4e-5 on the eval output after five steps).
Both are held to one error model: an fp32 contraction of n terms is off by at most n * 2^-24 of the sum of its terms' magnitudes, the
longest contraction here has D = 48 terms, and a value passes through about ten such layers, so a quantity is good to
U = 64 * 2^-23 of the scale of its kind (the largest gradient entry, the largest loss, the largest norm).  The eval output comes after
five Adam steps, whose update lr * m / (sqrt(v) + eps) has magnitude lr whatever the gradient's size: where the true gradient is 0 (the
three encoder biases: BatchNorm removes them) its direction is rounding noise, so parameters may differ by 5 lr = 5e-3 there, and the
output is held to 1e-3 of its scale only."""
import os
import re

import numpy as np
import pytest
import torch

import _diffusion_train_oracle as oracle_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 64 * 2.0 ** -23


@pytest.fixture(scope="module")
def fx():
    return oracle_mod.load_fixture()


@pytest.fixture(scope="module")
def runs(fx):
    return {(d, p): oracle_mod.fixture_run(fx, d, p) for d in (torch.float32, torch.float64) for p in ("", "noclip/")}


def test_fixture_is_small_and_holds_arrays_only(fx):
    assert os.path.getsize(oracle_mod.FIXTURE) < 256 * 1024
    assert all(isinstance(v, np.ndarray) and v.dtype.kind in "fi" for v in fx.values())
    assert tuple(fx["dims"][:6]) == (6, 48, 32, 32, 2, 10)
    assert fx["norm"].min() > 1.0, "the clip must be active in the clipped run"
    assert fx["init/norm.num_batches_tracked"] == 0 and fx["final/norm.num_batches_tracked"] == 5


@pytest.mark.parametrize("prefix", ["", "noclip/"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_oracle_reproduces_losses_and_norms(fx, runs, dtype, prefix):
    r = runs[(dtype, prefix)]
    dl = np.abs(np.array(r["loss"]) - fx[prefix + "loss"].astype(np.float64))
    dn = np.abs(np.array(r["norm"]) - fx[prefix + "norm"].astype(np.float64))
    print(f"{dtype} {prefix!r}: loss dev {dl.max():.3g}, norm dev {dn.max():.3g}")
    assert dl.max() <= U * fx[prefix + "loss"].max()
    assert dn.max() <= U * fx[prefix + "norm"].max()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_oracle_reproduces_step0_gradients(fx, runs, dtype):
    g = runs[(dtype, "")]["grad0"]
    keys = [k[len("grad0/"):] for k in fx if k.startswith("grad0/")]
    assert sorted(keys) == sorted(g) and len(keys) == 29
    worst, scale = 0.0, max(float(np.abs(fx["grad0/" + k]).max()) for k in keys)
    for k in keys:
        d = float(np.abs(g[k].double().numpy() - fx["grad0/" + k].astype(np.float64)).max())
        worst = max(worst, d)
        assert d <= U * scale, (k, d)
    print(f"{dtype}: worst step-0 gradient deviation {worst:.3g}")


def test_oracle_eval_output(fx, runs):
    for prefix in ("", "noclip/"):
        d = np.abs(runs[(torch.float64, prefix)]["eval_out"].numpy() - fx[prefix + "eval_out"].astype(np.float64)).max()
        print(f"{prefix!r}: eval output deviation {d:.3g}")
        assert d <= 1e-3 * np.abs(fx[prefix + "eval_out"]).max()


def test_abi_symbols_and_header():
    from nested_diffusion_amd import _lib, build
    names = ["nd_bn_train_fwd", "nd_bn_train_bwd", "nd_qsample", "nd_mse_grad", "nd_sumsq", "nd_sumsq_plan", "nd_sumsq_workspace_bytes",
             "nd_clip_adam"]
    with open(os.path.join(ROOT, "include", "nested_diffusion.h")) as f:
        header = f.read()
    for n in names:
        assert n in _lib.SIGNATURES, n
        assert re.search(r"\b(int|size_t) " + n + r"\(", header), n
    assert "nd_diffusion_train.hip" in build.SOURCES
    assert "ND_SUMSQ_CHUNK 4096" in header
    if os.path.exists(_lib.LIB_PATH):
        import ctypes
        lib = ctypes.CDLL(_lib.LIB_PATH) if not torch.cuda.is_available() else _lib.load()
        for n in names:
            assert hasattr(lib, n), n


def test_sumsq_plan_is_host_only():
    from nested_diffusion_amd import ops
    assert ops.sumsq_plan(1) == {"chunks": 1, "chain": 16 + 8 + 1 + 8 + 1}
    assert ops.sumsq_plan(4097)["chunks"] == 2
    p = ops.sumsq_plan(1_000_003)
    assert p["chunks"] == 245 and p["chain"] == 16 + 8 + 1 + 8 + 1
    assert ops.sumsq_plan(4096 * 257)["chain"] == 16 + 8 + 2 + 8 + 1


def _args(B=6, D=48, C=2, T=10, t=None):
    t = torch.arange(B, dtype=torch.int64) % T if t is None else t
    return (torch.zeros(B, D), torch.zeros(B, C), torch.zeros(B, C), t, torch.zeros(B, C), D, C, T)


def test_check_step_args_accepts_and_refuses():
    from nested_diffusion_amd.train_diffusion import check_step_args
    assert check_step_args(*_args()) == 6
    assert check_step_args(*_args(B=2)) == 2
    assert check_step_args(*_args(B=128)) == 128
    assert check_step_args(*_args(t=torch.tensor([0, 9, 0, 9, 5, 5]))) == 6
    bad = {"B = 1": _args(B=1), "B = 129": _args(B=129), "t == T": _args(t=torch.tensor([0, 1, 2, 10, 4, 5])),
           "t < 0": _args(t=torch.tensor([0, 1, -1, 3, 4, 5])), "int32 t": _args(t=torch.arange(6, dtype=torch.int32)),
           "rows of t": _args(t=torch.arange(5, dtype=torch.int64)), "float64 x": (torch.zeros(6, 48, dtype=torch.float64),) + _args()[1:],
           "D": (torch.zeros(6, 32),) + _args()[1:], "e rows": _args()[:4] + (torch.zeros(5, 2),) + _args()[5:]}
    for what, a in bad.items():
        with pytest.raises(ValueError):
            check_step_args(*a)
            pytest.fail(what)


def test_parser_has_mlp_idx():
    from nested_diffusion_amd.main import build_parser
    a = build_parser().parse_args(["--config", "c.yml", "--doc", "d", "--preprocess", "grayscaled", "--mlp_idx", "3"])
    assert a.mlp_idx == 3
