"""Host-side checks of the mapping-MLP training path (no GPU): the ABI carries nd_linear_wgrad_adam, nd_bias_grad_adam and nd_unpack_rows and
they refuse bad arguments before any launch, adam_step forms the bias corrections in double, StepLR and the CLI defaults are the
reference's numbers, and the Adam listing the kernels implement (restated here in numpy float32, one rounded operation per line) follows
torch.optim.Adam."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nd_linear_wgrad_adam", "nd_bias_grad_adam", "nd_unpack_rows", "nd_linear_wgrad_plan")
ADAM_FIELDS = ("beta1", "one_minus_beta1", "beta2", "one_minus_beta2", "step_size", "sqrt_bc2", "eps")


def adam_f32(w, m, v, g, a):
    """The listing of include/nested_diffusion.h (torch 1.10 F.adam) on numpy float32 arrays: every line is one rounded fp32 operation per
    element, numpy's sqrt and division are correctly rounded.  a: an ops.adam_step(...) (or anything with its seven fields).
    Returns the new (w, m, v)."""
    f = {k: np.float32(getattr(a, k)) for k in ADAM_FIELDS}
    w, m, v, g = (np.asarray(t, dtype=np.float32) for t in (w, m, v, g))
    m = (m * f["beta1"]) + (g * f["one_minus_beta1"])
    v = (v * f["beta2"]) + ((g * g) * f["one_minus_beta2"])
    denom = (np.sqrt(v) / f["sqrt_bc2"]) + f["eps"]
    w = w - f["step_size"] * (m / denom)
    assert w.dtype == m.dtype == v.dtype == np.float32
    return w, m, v


def test_header_library_and_ctypes_table_carry_the_entry_points():
    from nested_diffusion_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "nested_diffusion.h")).read()
    for name in SYMBOLS:
        decl = re.search(rf"\bint {name}\(([^;]*)\);", header)
        assert decl, name
        n_args = len([a for a in decl.group(1).split(",") if a.strip()])
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args, name
    struct = re.search(r"typedef struct nd_adam_step \{\s*float ([^;]*);\s*\} nd_adam_step;", header)
    assert struct and tuple(s.strip() for s in struct.group(1).split(",")) == ADAM_FIELDS
    assert tuple(n for n, _ in _lib.NdAdamStep._fields_) == ADAM_FIELDS and all(t is ctypes.c_float for _, t in _lib.NdAdamStep._fields_)
    assert "nd_mlp_train.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "nd_mlp_train.hip"))
    lib = ctypes.CDLL(build.build())
    for name in SYMBOLS:
        assert hasattr(lib, name), name


P = 0x10000          # a non-NULL, 16-byte aligned address: every case below is refused before anything is dereferenced or launched


def _refused(rc, lib, *words):
    msg = lib.nd_last_error().decode()
    assert rc == -1, (rc, msg)                                # ND_ERR_ARG
    for w in words:
        assert w in msg, (w, msg)


def test_entry_points_validate_their_arguments_without_a_gpu():
    from nested_diffusion_amd import _lib
    lib = _lib.load()
    a = ctypes.byref(_lib.NdAdamStep(0.9, 0.1, 0.999, 0.001, 1e-3, 1.0, 1e-8))
    F32, F16 = _lib.ND_DTYPE_F32, _lib.ND_DTYPE_F16
    wg = lib.nd_linear_wgrad_adam
    _refused(wg(None, P, P, P + 64, P + 128, None, 4, 16, 16, F32, 1.0, a, None), lib, "NULL", "dy")
    _refused(wg(P, None, P, P + 64, P + 128, None, 4, 16, 16, F32, 1.0, a, None), lib, "NULL", "x")
    _refused(wg(P, P, None, P + 64, P + 128, None, 4, 16, 16, F32, 1.0, a, None), lib, "NULL", "w_packed")
    _refused(wg(P, P, P, None, P + 128, None, 4, 16, 16, F32, 1.0, a, None), lib, "NULL", "m_packed")
    _refused(wg(P, P, P, P + 64, None, None, 4, 16, 16, F32, 1.0, a, None), lib, "NULL", "v_packed")
    _refused(wg(P, P, P, P + 64, P + 128, None, 0, 16, 16, F32, 1.0, a, None), lib, "M=0")
    _refused(wg(P, P, P, P + 64, P + 128, None, 129, 16, 16, F32, 1.0, a, None), lib, "M=129", "128")
    _refused(wg(P, P, P, P + 64, P + 128, None, 4, 16, 24, F32, 1.0, a, None), lib, "K=24", "16")
    _refused(wg(P, P, P, P + 64, P + 128, None, 4, 0, 16, F32, 1.0, a, None), lib, "N=0")
    _refused(wg(P, P, P, P + 64, P + 128, None, 4, 16, 32, F16, 1.0, a, None), lib, "dtype", "fp16")
    _refused(wg(P, P, P, P + 64, P + 128, None, 4, 16, 16, F32, 1.0, None, None), lib, "a and g_out")
    _refused(wg(P, P, P, P, P + 128, None, 4, 16, 16, F32, 1.0, a, None), lib, "distinct")
    _refused(wg(P, P, P + 4, P + 64, P + 128, None, 4, 16, 16, F32, 1.0, a, None), lib, "misaligned")
    bg = lib.nd_bias_grad_adam
    _refused(bg(None, P, P + 64, P + 128, None, 4, 16, 1.0, a, None), lib, "NULL", "dy")
    _refused(bg(P, None, P + 64, P + 128, None, 4, 16, 1.0, a, None), lib, "NULL", " b")
    _refused(bg(P, P, None, P + 128, None, 4, 16, 1.0, a, None), lib, "NULL", " m")
    _refused(bg(P, P, P + 64, None, None, 4, 16, 1.0, a, None), lib, "NULL", " v")
    _refused(bg(P, P, P + 64, P + 128, None, 0, 16, 1.0, a, None), lib, "M=0")
    _refused(bg(P, P, P + 64, P + 128, None, 4, 0, 1.0, a, None), lib, "N=0")
    _refused(bg(P, P, P + 64, P + 128, None, 4, 16, 1.0, None, None), lib, "a and g_out")
    up = lib.nd_unpack_rows
    _refused(up(None, P, 4, 16, F32, None), lib, "NULL", "src_packed")
    _refused(up(P, None, 4, 16, F32, None), lib, "NULL", "dst")
    _refused(up(P, P + 4096, 0, 16, F32, None), lib, "R=0")
    _refused(up(P, P + 4096, 4, 24, F32, None), lib, "K=24")
    _refused(up(P, P + 4096, 4, 32, F16, None), lib, "dtype", "fp32")
    out = (ctypes.c_int * 4)()
    _refused(lib.nd_linear_wgrad_plan(16, 24, out), lib, "K=24")
    _refused(lib.nd_linear_wgrad_plan(16, 16, None), lib, "NULL")


def test_wgrad_plan_covers_every_block_once():
    """grid.x * blocks-per-workgroup covers K / 16, grid.y * row-blocks-per-workgroup covers ceil(N / 16), with no empty workgroup row"""
    from nested_diffusion_amd import ops
    for N, K in ((1, 16), (2, 16), (17, 48), (128, 2048), (2048, 4096), (4096, 150528), (11205, 304)):
        p = ops.linear_wgrad_plan(N, K)
        nkb, nrb = K // 16, (N + 15) // 16
        assert (p["grid_x"] - 1) * p["kb_per_wg"] < nkb <= p["grid_x"] * p["kb_per_wg"], (N, K, p)
        assert (p["grid_y"] - 1) * p["rb_per_wg"] < nrb <= p["grid_y"] * p["rb_per_wg"], (N, K, p)
        assert 1 <= p["grid_y"] <= 65535


def test_adam_step_forms_the_bias_corrections_in_double():
    from nested_diffusion_amd import ops
    for t, bc1, bc2 in ((1, 1 - 0.9, 1 - 0.999), (2, 1 - 0.9 ** 2, 1 - 0.999 ** 2), (1000, 1 - 0.9 ** 1000, 1 - 0.999 ** 1000)):
        a = ops.adam_step(1e-3, t)
        assert a.step_size == np.float32(1e-3 / bc1) and a.sqrt_bc2 == np.float32(math.sqrt(bc2)), t
        assert a.beta1 == np.float32(0.9) and a.one_minus_beta1 == np.float32(1 - 0.9) and a.beta2 == np.float32(0.999)
        assert a.one_minus_beta2 == np.float32(1 - 0.999) and a.eps == np.float32(1e-8)
    # the values themselves: t = 1 gives lr / 0.1 and sqrt(0.001); at t = 1000 beta1^t has vanished and 1 - beta2^t = 0.6323...
    assert ops.adam_step(1e-3, 1).step_size == pytest.approx(1e-2, rel=1e-6) and ops.adam_step(1e-3, 1).sqrt_bc2 == pytest.approx(0.0316227766, rel=1e-6)
    assert ops.adam_step(1e-3, 2).step_size == pytest.approx(1e-3 / 0.19, rel=1e-6)
    assert ops.adam_step(5e-4, 1000).step_size == np.float32(5e-4) and ops.adam_step(5e-4, 1000).sqrt_bc2 == pytest.approx(0.7951758, rel=1e-6)
    # a float32 1 - beta2^t would be off in the 7th digit at t = 1: the double form is what torch's Python computes
    assert ops.adam_step(1e-3, 1).sqrt_bc2 != np.float32(math.sqrt(np.float32(1) - np.float32(0.999)))
    b = ops.adam_step(0.0, 3, betas=(0.5, 0.75), eps=1e-6)
    assert (b.beta1, b.one_minus_beta1, b.beta2, b.one_minus_beta2, b.step_size) == (0.5, 0.5, 0.75, 0.25, 0.0)
    for bad in (dict(t=0), dict(t=1, betas=(1.0, 0.999)), dict(t=1, lr=-1.0)):
        with pytest.raises(ValueError):
            ops.adam_step(**{"lr": 1e-3, **bad})


def test_step_lr_and_cli_defaults_are_the_references_numbers():
    from nested_diffusion_amd import train_mapping as tm
    assert tm.step_lr(1e-3, 0, 20, 0.5) == 1e-3 and tm.step_lr(1e-3, 19, 20, 0.5) == 1e-3
    assert tm.step_lr(1e-3, 20, 20, 0.5) == 5e-4 and tm.step_lr(1e-3, 39, 20, 0.5) == 5e-4
    assert tm.step_lr(1e-3, 40, 20, 0.5) == 2.5e-4 and tm.step_lr(1e-3, 300, 20, 0.5) == 1e-3 * 0.5 ** 15
    assert tm.step_lr(5e-4, 99, 20, 0.5) == 5e-4 / 16
    w = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([w], lr=1e-3)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=20, gamma=0.5)
    for epoch in range(65):
        assert opt.param_groups[0]["lr"] == pytest.approx(tm.step_lr(1e-3, epoch, 20, 0.5), rel=1e-12), epoch
        opt.step()
        sched.step()
    assert tm.DATASET_DEFAULTS == {
        "ChestXRay": dict(num_classes=2, batch_size=30, lr=1e-3, step_size=20, gamma=0.5, epochs=301),
        "ISICSkinCancer": dict(num_classes=2, batch_size=30, lr=5e-4, step_size=20, gamma=0.5, epochs=100)}
    assert (tm.TRAIN_DIR, tm.VALID_DIR, tm.VALID_BATCH, tm.MAX_BATCH) == ("training", "validation", 70, 128)
    base = ["--root_dir", "r", "--mn_idx", "2", "--vit", "v.pth", "--out", "o"]
    a = tm.build_parser().parse_args(["--dataset", "ChestXRay", *base])
    assert vars(a) == {"seed": None, "dataset": "ChestXRay", "root_dir": "r", "preprocess": "grayscaled", "mn_idx": 2, "vit": "v.pth", "out": "o",
                       "epochs": None, "batch_size": None}
    s = tm.resolve_settings(a)
    assert 0 <= s.pop("seed") <= 10000 and s == tm.DATASET_DEFAULTS["ChestXRay"]
    b = tm.build_parser().parse_args(["--dataset", "ISICSkinCancer", "--seed", "7", "--epochs", "2", "--batch_size", "12", "--preprocess",
                                      "standardized", *base])
    assert tm.resolve_settings(b) == dict(num_classes=2, batch_size=12, lr=5e-4, step_size=20, gamma=0.5, epochs=2, seed=7)
    for bad in (["--dataset", "PathMNIST", *base], ["--dataset", "ChestXRay", "--root_dir", "r", "--mn_idx", "5", "--vit", "v", "--out", "o"],
                ["--dataset", "ChestXRay", "--root_dir", "r", "--mn_idx", "0", "--out", "o"]):
        with pytest.raises(SystemExit):
            tm.build_parser().parse_args(bad)
    with pytest.raises(SystemExit, match="128"):             # a batch the weight-gradient kernel cannot sum in one launch: refused by name
        tm.resolve_settings(tm.build_parser().parse_args(["--dataset", "ChestXRay", "--batch_size", "129", *base]))


def test_the_float32_listing_follows_torch_adam():
    """50 steps of a fixed gradient sequence: the numpy float32 listing against torch.optim.Adam in float32, within 4 x the deviation of that
    torch float32 run from a torch float64 run (the installed torch may order the same operations differently)."""
    from nested_diffusion_amd import ops
    g = torch.Generator().manual_seed(5)
    n, steps, lr = 256, 50, 1e-3
    w0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * (10.0 ** float(torch.randint(-3, 2, (1,), generator=g))) for _ in range(steps)]
    runs = {}
    for dt in (torch.float32, torch.float64):
        p = torch.nn.Parameter(w0.to(dt).clone())
        opt = torch.optim.Adam([p], lr=lr)
        for gr in grads:
            p.grad = gr.to(dt).clone()
            opt.step()
        runs[dt] = p.detach().double().numpy()
    w, m, v = w0.numpy().copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
    for t, gr in enumerate(grads, start=1):
        w, m, v = adam_f32(w, m, v, gr.numpy(), ops.adam_step(lr, t))
    yard = float(np.abs(runs[torch.float32] - runs[torch.float64]).max())
    dev = float(np.abs(w.astype(np.float64) - runs[torch.float32]).max())
    moved = float(np.abs(runs[torch.float64] - w0.double().numpy()).max())
    assert yard > 0.0 and moved > 10 * lr
    assert dev <= 4 * yard, f"listing vs torch float32: {dev:.3e}; yardstick (torch float32 vs float64): {yard:.3e}; parameters moved {moved:.3e}"
