"""Host-side checks of the ViT training path (no GPU): the ABI carries nd_gemm_tn_adamw, nd_gemm_tn_plan, nd_colsum_adamw and
nd_layernorm_wgrad_adamw and they refuse bad arguments before any launch, the plan covers every tile once, adamw_step forms its constants
in double, StepLR, the CLI defaults and the fresh model's statistics are the reference's, and the AdamW listing the kernels implement
(restated here in numpy float32, one rounded operation per line) follows torch.optim.AdamW."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nd_gemm_tn_adamw", "nd_colsum_adamw", "nd_layernorm_wgrad_adamw", "nd_gemm_tn_plan", "nd_layernorm_wgrad_workspace_bytes")
ADAMW_FIELDS = ("beta1", "one_minus_beta1", "beta2", "one_minus_beta2", "step_size", "sqrt_bc2", "eps", "decay")


def adamw_f32(w, m, v, g, a):
    """The listing of include/nested_diffusion.h (torch 1.10 F.adamw) on numpy float32 arrays: every line is one rounded fp32 operation
    per element, numpy's sqrt and division are correctly rounded.  a: an ops.adamw_step(...).  Returns the new (w, m, v)."""
    f = {k: np.float32(getattr(a, k)) for k in ADAMW_FIELDS}
    w, m, v, g = (np.asarray(t, dtype=np.float32) for t in (w, m, v, g))
    w = w * f["decay"]
    m = (m * f["beta1"]) + (g * f["one_minus_beta1"])
    v = (v * f["beta2"]) + ((g * g) * f["one_minus_beta2"])
    denom = (np.sqrt(v) / f["sqrt_bc2"]) + f["eps"]
    w = w - f["step_size"] * (m / denom)
    assert w.dtype == m.dtype == v.dtype == np.float32
    return w, m, v


def chunked_colsum_f32(terms, chunk):
    """The documented order of nd_colsum_adamw / nd_layernorm_wgrad_adamw on a float32 [rows, cols] array of terms: chunks of `chunk` rows,
    p = 0, p += term in row order; acc = 0, acc += p in chunk order."""
    terms = np.asarray(terms, dtype=np.float32)
    acc = np.zeros(terms.shape[1], np.float32)
    for r0 in range(0, terms.shape[0], chunk):
        p = np.zeros(terms.shape[1], np.float32)
        for r in range(r0, min(r0 + chunk, terms.shape[0])):
            p = p + terms[r]
        acc = acc + p
    return acc


def test_header_library_and_ctypes_table_carry_the_entry_points():
    from nested_diffusion_amd import _lib, build, ops
    header = open(os.path.join(ROOT, "include", "nested_diffusion.h")).read()
    for name in SYMBOLS:
        decl = re.search(rf"\b(?:int|size_t) {name}\(([^;]*)\);", header)
        assert decl, name
        n_args = len([a for a in decl.group(1).split(",") if a.strip()])
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args, name
    struct = re.search(r"typedef struct nd_adamw_step \{\s*float ([^;]*);\s*\} nd_adamw_step;", header)
    assert struct and tuple(s.strip() for s in struct.group(1).split(",")) == ADAMW_FIELDS
    assert tuple(n for n, _ in _lib.NdAdamwStep._fields_) == ADAMW_FIELDS and all(t is ctypes.c_float for _, t in _lib.NdAdamwStep._fields_)
    assert int(re.search(r"#define ND_COLSUM_CHUNK (\d+)", header).group(1)) == ops.COLSUM_CHUNK
    assert "nd_vit_train.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "nd_vit_train.hip"))
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
    a = ctypes.byref(_lib.NdAdamwStep(0.9, 0.1, 0.999, 0.001, 1e-3, 1.0, 1e-8, 1.0))
    w, m, v = P + 4096, P + 8192, P + 12288
    gt = lib.nd_gemm_tn_adamw
    _refused(gt(None, P, w, m, v, None, 4, 16, 16, 1.0, a, None), lib, "NULL", "dy")
    _refused(gt(P, None, w, m, v, None, 4, 16, 16, 1.0, a, None), lib, "NULL", " x")
    _refused(gt(P, P, None, m, v, None, 4, 16, 16, 1.0, a, None), lib, "NULL", " w")
    _refused(gt(P, P, w, None, v, None, 4, 16, 16, 1.0, a, None), lib, "NULL", " m")
    _refused(gt(P, P, w, m, None, None, 4, 16, 16, 1.0, a, None), lib, "NULL", " v")
    _refused(gt(P, P, w, m, v, None, 0, 16, 16, 1.0, a, None), lib, "M=0")
    _refused(gt(P, P, w, m, v, None, 4, 0, 16, 1.0, a, None), lib, "N=0")
    _refused(gt(P, P, w, m, v, None, 4, 16, 24, 1.0, a, None), lib, "K=24", "16")
    _refused(gt(P, P, w, m, v, None, 4, 16, 0, 1.0, a, None), lib, "K=0")
    _refused(gt(P, P, w, m, v, None, 4, 16, 16, 1.0, None, None), lib, "a and g_out")
    _refused(gt(P, P, None, None, None, None, 4, 16, 16, 1.0, None, None), lib, "a and g_out")
    _refused(gt(P, P, w, w, v, None, 4, 16, 16, 1.0, a, None), lib, "distinct")
    _refused(gt(P, P, w, m, v, w, 4, 16, 16, 1.0, a, None), lib, "distinct")
    _refused(gt(P, P, w + 2, m, v, None, 4, 16, 16, 1.0, a, None), lib, "misaligned")
    cs = lib.nd_colsum_adamw
    _refused(cs(None, w, m, v, None, 4, 16, 1.0, a, None), lib, "NULL", "dy")
    _refused(cs(P, None, m, v, None, 4, 16, 1.0, a, None), lib, "NULL", " b")
    _refused(cs(P, w, None, v, None, 4, 16, 1.0, a, None), lib, "NULL", " m")
    _refused(cs(P, w, m, None, None, 4, 16, 1.0, a, None), lib, "NULL", " v")
    _refused(cs(P, w, m, v, None, 0, 16, 1.0, a, None), lib, "M=0")
    _refused(cs(P, w, m, v, None, 4, 0, 1.0, a, None), lib, "N=0")
    _refused(cs(P, w, m, v, None, 4, 16, 1.0, None, None), lib, "a and g_out")
    _refused(cs(P, w, m, m, None, 4, 16, 1.0, a, None), lib, "distinct")
    ln = lib.nd_layernorm_wgrad_adamw
    st = [P + 4096 * i for i in range(2, 8)]                  # gamma, beta, m_gamma, v_gamma, m_beta, v_beta
    WS = P + 4096 * 9                                         # the workspace of per-chunk partials
    _refused(ln(None, P, *st, None, None, 4, 128, 1e-6, 1.0, a, WS, 1 << 20, None), lib, "NULL", " x")
    _refused(ln(P, None, *st, None, None, 4, 128, 1e-6, 1.0, a, WS, 1 << 20, None), lib, "NULL", " g")
    for i in range(6):
        holed = list(st)
        holed[i] = None
        _refused(ln(P, P + 4096, *holed, None, None, 4, 128, 1e-6, 1.0, a, WS, 1 << 20, None), lib, "NULL")
    _refused(ln(P, P + 4096, *st, None, None, 4, 128, 1e-6, 1.0, None, WS, 1 << 20, None), lib, "nothing to write")
    _refused(ln(P, P + 4096, *st, None, None, 0, 128, 1e-6, 1.0, a, WS, 1 << 20, None), lib, "rows=0")
    _refused(ln(P, P + 4096, *st, None, None, 4, 130, 1e-6, 1.0, a, WS, 1 << 20, None), lib, "dim=130")
    _refused(ln(P, P + 4096, *st, None, None, 4, 2052, 1e-6, 1.0, a, WS, 1 << 20, None), lib, "dim=2052", "2048")
    _refused(ln(P, P + 4096, st[0], st[0], *st[2:], None, None, 4, 128, 1e-6, 1.0, a, WS, 1 << 20, None), lib, "distinct")
    _refused(ln(P + 4, P + 4096, *st, None, None, 4, 128, 1e-6, 1.0, a, WS, 1 << 20, None), lib, "misaligned")
    wsb = lib.nd_layernorm_wgrad_workspace_bytes
    assert wsb(4, 128) == 2 * 128 * 4 and wsb(64, 128) == 2 * 128 * 4 and wsb(65, 128) == 2 * 2 * 128 * 4 and wsb(5910, 768) == 93 * 2 * 768 * 4
    assert wsb(0, 128) == 0 and wsb(4, 130) == 0 and wsb(4, 2052) == 0
    _refused(ln(P, P + 4096, *st, None, None, 65, 128, 1e-6, 1.0, a, WS, wsb(65, 128) - 1, None), lib, "workspace", "2048 needed")
    _refused(ln(P, P + 4096, *st, None, None, 4, 128, 1e-6, 1.0, a, None, 1 << 20, None), lib, "workspace")
    _refused(ln(P, P + 4096, *st, None, None, 4, 128, 1e-6, 1.0, a, WS + 4, 1 << 20, None), lib, "misaligned")
    out = (ctypes.c_int * 5)()
    _refused(lib.nd_gemm_tn_plan(16, 24, out), lib, "K=24")
    _refused(lib.nd_gemm_tn_plan(0, 16, out), lib, "N=0")
    _refused(lib.nd_gemm_tn_plan(16, 16, None), lib, "NULL")


@pytest.mark.parametrize("N,K", [(1, 16), (2, 128), (17, 48), (768, 768), (2304, 768), (768, 3072)])
def test_gemm_tn_plan_covers_every_tile_exactly_once(N, K):
    from nested_diffusion_amd import ops
    p = ops.gemm_tn_plan(N, K)
    assert p["tile_n"] % 16 == 0 and p["tile_k"] % 16 == 0 and p["m_tile"] % 4 == 0 and p["m_tile"] >= 4
    assert 1 <= p["grid_n"] <= 65535 and p["grid_k"] >= 1
    count = np.zeros((N, K), np.int32)                        # workgroup (by, bx) owns rows [by tile_n, ...) x columns [bx tile_k, ...)
    for by in range(p["grid_n"]):
        for bx in range(p["grid_k"]):
            n0, k0 = by * p["tile_n"], bx * p["tile_k"]
            assert n0 < N and k0 < K, (by, bx, p)                 # no empty workgroup
            count[n0:n0 + p["tile_n"], k0:k0 + p["tile_k"]] += 1
    assert bool((count == 1).all())


def test_adamw_step_forms_decay_and_the_bias_corrections_in_double():
    from nested_diffusion_amd import ops
    for t, bc1, bc2 in ((1, 1 - 0.9, 1 - 0.999), (2, 1 - 0.9 ** 2, 1 - 0.999 ** 2), (1000, 1 - 0.9 ** 1000, 1 - 0.999 ** 1000)):
        a = ops.adamw_step(1e-4, t)
        assert a.step_size == np.float32(1e-4 / bc1) and a.sqrt_bc2 == np.float32(math.sqrt(bc2)), t
        assert a.beta1 == np.float32(0.9) and a.one_minus_beta1 == np.float32(1 - 0.9) and a.beta2 == np.float32(0.999)
        assert a.one_minus_beta2 == np.float32(1 - 0.999) and a.eps == np.float32(1e-8)
        assert a.decay == np.float32(1 - 1e-4 * 0.1)
    # 1 - lr * wd formed in float32 from float32 factors is another number: the double form is what torch's Python computes
    assert ops.adamw_step(1e-4, 1).decay == pytest.approx(0.99999, rel=1e-7)
    assert ops.adamw_step(3e-4, 1, weight_decay=0.3).decay == np.float32(1 - 3e-4 * 0.3)
    assert ops.adamw_step(1e-4, 1).sqrt_bc2 != np.float32(math.sqrt(np.float32(1) - np.float32(0.999)))
    assert ops.adamw_step(0.0, 3).decay == 1.0 and ops.adamw_step(0.0, 3).step_size == 0.0
    assert ops.adamw_step(1e-4, 5, weight_decay=0.0).decay == 1.0
    b = ops.adamw_step(0.5, 3, weight_decay=0.5, betas=(0.5, 0.75), eps=1e-6)
    assert (b.beta1, b.one_minus_beta1, b.beta2, b.one_minus_beta2, b.decay) == (0.5, 0.5, 0.75, 0.25, 0.75)
    for bad in (dict(t=0), dict(t=1, betas=(1.0, 0.999)), dict(t=1, lr=-1.0), dict(t=1, weight_decay=-0.1)):
        with pytest.raises(ValueError):
            ops.adamw_step(**{"lr": 1e-4, **bad})


def test_the_float32_listing_follows_torch_adamw():
    """50 steps of a fixed gradient sequence: the numpy float32 listing against torch.optim.AdamW in float32, within 4 x the deviation of
    that torch float32 run from a torch float64 run (the installed torch may order the same operations differently)."""
    from nested_diffusion_amd import ops
    g = torch.Generator().manual_seed(5)
    n, steps, lr, wd = 256, 50, 1e-3, 0.1
    w0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * (10.0 ** float(torch.randint(-3, 2, (1,), generator=g))) for _ in range(steps)]
    runs = {}
    for dt in (torch.float32, torch.float64):
        p = torch.nn.Parameter(w0.to(dt).clone())
        opt = torch.optim.AdamW([p], lr=lr, weight_decay=wd)
        for gr in grads:
            p.grad = gr.to(dt).clone()
            opt.step()
        runs[dt] = p.detach().double().numpy()
    w, m, v = w0.numpy().copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
    for t, gr in enumerate(grads, start=1):
        w, m, v = adamw_f32(w, m, v, gr.numpy(), ops.adamw_step(lr, t, wd))
    yard = float(np.abs(runs[torch.float32] - runs[torch.float64]).max())
    dev = float(np.abs(w.astype(np.float64) - runs[torch.float32]).max())
    moved = float(np.abs(runs[torch.float64] - w0.double().numpy()).max())
    # the decay is really in the listing: plain Adam ends elsewhere
    plain = torch.nn.Parameter(w0.double().clone())
    opt = torch.optim.Adam([plain], lr=lr)
    for gr in grads:
        plain.grad = gr.double().clone()
        opt.step()
    assert float(np.abs(plain.detach().numpy() - runs[torch.float64]).max()) > 100 * max(yard, 1e-9)
    assert yard > 0.0 and moved > 10 * lr
    assert dev <= 4 * yard, f"listing vs torch float32: {dev:.3e}; yardstick (torch float32 vs float64): {yard:.3e}; parameters moved {moved:.3e}"


def test_step_lr_and_cli_defaults_are_the_references_numbers():
    from nested_diffusion_amd import train_transformer as tt
    assert tt.step_lr(1e-4, 0, 10, 0.5) == 1e-4 and tt.step_lr(1e-4, 9, 10, 0.5) == 1e-4
    assert tt.step_lr(1e-4, 10, 10, 0.5) == 5e-5 and tt.step_lr(1e-4, 199, 10, 0.5) == 1e-4 * 0.5 ** 19
    w = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.AdamW([w], lr=1e-4, weight_decay=0.1)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=10, gamma=0.5)
    for epoch in range(35):
        assert opt.param_groups[0]["lr"] == pytest.approx(tt.step_lr(1e-4, epoch, 10, 0.5), rel=1e-12), epoch
        opt.step()
        sched.step()
    ref = dict(num_classes=2, batch_size=30, lr=1e-4, weight_decay=0.1, step_size=10, gamma=0.5, epochs=200)
    assert tt.DATASET_DEFAULTS == {"ChestXRay": ref, "ISICSkinCancer": ref}
    assert tt.checkpoint_path("o", "ChestXRay") == os.path.join("o", "vit_base_patch16_224_ChestXRay.pth")
    base = ["--root_dir", "r", "--out", "o"]
    a = tt.build_parser().parse_args(["--dataset", "ChestXRay", *base])
    assert vars(a) == {"seed": None, "dataset": "ChestXRay", "root_dir": "r", "preprocess": "grayscaled", "out": "o", "init": None,
                       "epochs": None, "batch_size": None}
    s = tt.resolve_settings(a)
    assert 0 <= s.pop("seed") <= 10000 and s == ref
    b = tt.build_parser().parse_args(["--dataset", "ISICSkinCancer", "--seed", "7", "--epochs", "2", "--batch_size", "200", "--preprocess",
                                      "standardized", "--init", "c.pth", *base])
    assert tt.resolve_settings(b) == {**ref, "batch_size": 200, "epochs": 2, "seed": 7}      # no 128-row limit on the batch
    for bad in (["--dataset", "PathMNIST", *base], ["--dataset", "ChestXRay", "--root_dir", "r"], ["--dataset", "ChestXRay", "--out", "o"]):
        with pytest.raises(SystemExit):
            tt.build_parser().parse_args(bad)
    with pytest.raises(SystemExit):
        tt.resolve_settings(tt.build_parser().parse_args(["--dataset", "ChestXRay", "--batch_size", "0", *base]))
    # the trainer's signature carries the reference's optimizer settings as its defaults
    import inspect
    d = {k: p.default for k, p in inspect.signature(tt.ViTTrainer.__init__).parameters.items()}
    assert (d["lr"], d["weight_decay"], d["step_size"], d["gamma"]) == (1e-4, 0.1, 10, 0.5)


def test_fresh_model_has_the_stated_statistics():
    from nested_diffusion_amd import train_transformer as tt
    embed, depth, C = 128, 2, 3
    sd = tt.init_state_dict(num_classes=C, embed=embed, depth=depth, patch=16, img=32, seed=4)
    keys = ["cls_token", "pos_embed", "patch_embed.proj.weight", "patch_embed.proj.bias"]
    for i in range(depth):
        keys += [f"blocks.{i}.{n}.{s}" for n in ("norm1", "attn.qkv", "attn.proj", "norm2", "mlp.fc1", "mlp.fc2") for s in ("weight", "bias")]
    keys += ["norm.weight", "norm.bias", "head.weight", "head.bias"]
    assert list(sd) == keys                                   # timm's state-dict order
    assert sd["cls_token"].shape == (1, 1, embed) and sd["pos_embed"].shape == (1, 5, embed)
    assert sd["patch_embed.proj.weight"].shape == (embed, 3, 16, 16) and sd["head.weight"].shape == (C, embed)
    assert sd["blocks.0.attn.qkv.weight"].shape == (3 * embed, embed) and sd["blocks.1.mlp.fc2.weight"].shape == (embed, 4 * embed)
    cut = float(np.float32(2 * 0.02))
    normals = []
    for k, t in sd.items():
        assert t.dtype == torch.float32
        if "norm" in k:
            assert bool((t == (1.0 if k.endswith("weight") else 0.0)).all()), k
        elif k.startswith("blocks.") and k.endswith("bias"):
            assert bool((t == 0).all()), k
        elif k.startswith("blocks.") or k in ("cls_token", "pos_embed"):
            assert float(t.abs().max()) <= cut, k
            normals.append(t.flatten())
    allw = torch.cat(normals).double()
    # a normal of std 0.02 cut at two standard deviations has std 0.02 * 0.8796; the sample has ~4e5 values
    assert abs(float(allw.mean())) < 2e-4 and float(allw.std()) == pytest.approx(0.02 * 0.8796, rel=0.01)
    assert float(allw.abs().max()) > 0.039                    # and it is cut at 2 sigma, not far inside
    for k, fan in (("patch_embed.proj.weight", 3 * 16 * 16), ("patch_embed.proj.bias", 3 * 16 * 16), ("head.weight", embed), ("head.bias", embed)):
        b = 1.0 / math.sqrt(fan)
        assert float(sd[k].abs().max()) <= float(np.float32(b)), k
        if sd[k].numel() > 1000:
            assert float(sd[k].double().std()) == pytest.approx(b / math.sqrt(3.0), rel=0.02) and float(sd[k].abs().max()) > 0.99 * b
    again = tt.init_state_dict(num_classes=C, embed=embed, depth=depth, patch=16, img=32, seed=4)
    other = tt.init_state_dict(num_classes=C, embed=embed, depth=depth, patch=16, img=32, seed=5)
    assert all(torch.equal(sd[k], again[k]) for k in sd) and not torch.equal(sd["head.weight"], other["head.weight"])


def test_trainer_refuses_the_other_arithmetic_modes_by_name(monkeypatch):
    """fp16 mode and the f32-input-MFMA form of the ViT GEMMs hold no frag32b3 images to train behind: refused before anything is built"""
    from nested_diffusion_amd import _lib
    from nested_diffusion_amd import train_transformer as tt
    with pytest.raises(_lib.NdError, match="fp16"):
        tt.ViTTrainer(None, dtype="f16")
    monkeypatch.setenv("ND_GEMM_F32", "mfma_f32")
    with pytest.raises(_lib.NdError, match="ND_GEMM_F32=mfma_f32"):
        tt.ViTTrainer(None)
