"""Host-side pieces of the adversarial path: the Linf attack table, the refused attacks, the attacked-dataset reader and the C ABI
declarations of the gradient kernels (no GPU needed)."""
import math
import os
import re
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["nd_layernorm_bwd", "nd_gelu_split", "nd_gelu_bwd_split", "nd_attention_bwd", "nd_xent_head_bwd", "nd_unpatchify",
               "nd_linf_step", "nd_linf_random_start"]


def test_linf_attack_table():
    from nested_diffusion_amd import attack
    fake = types.SimpleNamespace(device="cpu")
    want = {"FGSM": ("LinfFastGradientAttack", 1.0, 1, False), "PGD": ("LinfProjectedGradientDescentAttack", 0.01 / 0.3, 40, True),
            "LinfBIM": ("LinfBasicIterativeAttack", 0.2, 10, False)}
    assert attack.LINF_ATTACKS == want
    for name, (_, rel, steps, rs) in want.items():
        a = attack.Attack(8 / 255, name, fake)
        assert (a.steps, a.random_start) == (steps, rs)
        assert math.isclose(a.stepsize, rel * 8 / 255)
    assert attack.BOUNDS == (0.0, 1.0)
    # a GuidingConditioner is accepted for its ViT (the reference attacks cond_pred_model['vit'])
    assert attack.Attack(0.1, "FGSM", types.SimpleNamespace(vit=fake)).model is fake


@pytest.mark.parametrize("name", ["CW", "BIM", "L2PGD", "AUTOPGD"])
def test_unimplemented_attacks_name_themselves(name):
    from nested_diffusion_amd import attack
    with pytest.raises(NotImplementedError, match=name):
        attack.Attack(0.1, name, types.SimpleNamespace(device="cpu"))


def test_unknown_attack_is_rejected():
    from nested_diffusion_amd import attack
    with pytest.raises(ValueError):
        attack.Attack(0.1, "Nope", types.SimpleNamespace(device="cpu"))
    with pytest.raises(NotImplementedError, match="AUTOPGD"):
        attack.apply_attack(None, torch.zeros(1), torch.zeros(1), "AUTOPGD")


def _png_tree(root, name, size=(40, 30)):
    from PIL import Image
    rng = np.random.default_rng(0)
    d = os.path.join(root, f"Test_attacks_{name}")
    files = {}
    for cls in ("NORMAL", "PNEUMONIA"):
        os.makedirs(os.path.join(d, cls))
        for k in range(2):
            a = rng.integers(0, 256, size=(size[1], size[0], 3), dtype=np.uint8)
            p = os.path.join(d, cls, f"img{k}.png")
            Image.fromarray(a, "RGB").save(p)
            files[(cls, k)] = a
    return files


@pytest.mark.parametrize("dataset", ["ChestXRayAtkFGSM", "ISICSkinCancerAtkPGD"])
def test_get_dataset_reads_the_attacked_tree(tmp_path, dataset):
    from PIL import Image
    from nested_diffusion_amd import data
    attack_name = dataset.split("Atk")[1]
    files = _png_tree(str(tmp_path), attack_name)
    cfg = types.SimpleNamespace(data=types.SimpleNamespace(dataset=dataset, dataroot=str(tmp_path)))
    ds = data.get_dataset(types.SimpleNamespace(preprocess="grayscaled"), cfg)
    assert ds.classes == ["NORMAL", "PNEUMONIA"] and len(ds) == 4
    x, t = ds[2]
    assert t == 1 and x.shape == (3, 224, 224)
    # RGB, Resize((224, 224)) bilinear, ToTensor: no grayscale, no Normalize
    want = np.array(Image.fromarray(files[("PNEUMONIA", 0)], "RGB").resize((224, 224), Image.BILINEAR), dtype=np.uint8)
    assert torch.equal(x, torch.from_numpy(want).permute(2, 0, 1).float().div(255))
    assert not torch.equal(x[0], x[1])                      # colour survives (grayscaled would make the channels equal)


def test_all_ten_attacked_names_are_accepted():
    from nested_diffusion_amd import data
    names = {f"{d}Atk{a}" for d in ("ChestXRay", "ISICSkinCancer") for a in ("FGSM", "PGD", "BIM", "AUTOPGD", "CW")}
    assert set(data.ATTACKED_DATASETS) == names


def test_header_and_signatures_carry_the_gradient_entry_points():
    from nested_diffusion_amd import _lib
    with open(os.path.join(ROOT, "include", "nested_diffusion.h")) as f:
        hdr = f.read()
    for s in NEW_SYMBOLS:
        assert re.search(rf"\bint {s}\(", hdr), s
        assert s in _lib.SIGNATURES, s
    assert "ND_LINF_START_TAG 0x41544B31u" in hdr
    from nested_diffusion_amd import build
    assert "nd_vit_grad.hip" in build.SOURCES
    assert "nd_attack_linf.hip" in build.SOURCES


def test_every_csrc_header_is_a_build_dependency():
    """is_stale() looks at build.HEADERS: every header under csrc/ is in it, so a new one cannot be forgotten."""
    from nested_diffusion_amd import build
    csrc = os.path.join(ROOT, "nested_diffusion_amd", "csrc")
    hpp = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hpp")]
    assert "nd_philox.hpp" in map(os.path.basename, hpp) and set(hpp) <= set(build.HEADERS)
    assert os.path.join(ROOT, "include", "nested_diffusion.h") in build.HEADERS


def test_every_csrc_unit_is_a_build_source():
    """build.SOURCES is exactly the *.hip files under csrc/, and every per-unit flag of build.EXTRA_FLAGS names one of them: a renamed
    unit cannot be left out of the library or silently lose its flag."""
    from nested_diffusion_amd import build
    hip = {f for f in os.listdir(os.path.join(ROOT, "nested_diffusion_amd", "csrc")) if f.endswith(".hip")}
    assert hip == set(build.SOURCES) and len(build.SOURCES) == len(hip)
    assert set(build.EXTRA_FLAGS) <= set(build.SOURCES)


def test_one_philox_under_csrc():
    """The Philox multiplier stands in exactly one file under csrc/: every random draw of the library goes through one generator."""
    csrc = os.path.join(ROOT, "nested_diffusion_amd", "csrc")
    holders = []
    for f in sorted(os.listdir(csrc)):
        with open(os.path.join(csrc, f)) as fh:
            if "d2511f53" in fh.read().lower():
                holders.append(f)
    assert holders == ["nd_philox.hpp"]


def test_gradient_kernels_refuse_bad_arguments_before_any_launch():
    """The argument checks of the gradient / attack entry points return ND_ERR_ARG with an nd_last_error text before any HIP call
    (dummy non-NULL pointers: nothing is dereferenced)."""
    from nested_diffusion_amd import _lib, build
    build.build()
    lib = _lib.load()
    P = 4096                                                       # a dummy non-NULL address, never dereferenced
    cases = [
        (lambda: lib.nd_attention_bwd(P, P, P, P, None, 2, 0, 12, None), rb"1 <= N <= 208.*N=0"),
        (lambda: lib.nd_attention_bwd(P, P, P, P, None, 2, 209, 12, None), rb"1 <= N <= 208.*N=209"),
        (lambda: lib.nd_attention_bwd(P, P, P, P, None, 2, 197, 0, None), rb"heads >= 1"),
        (lambda: lib.nd_layernorm_bwd(P, P, P, None, P, None, 4, 6, 1e-6, None), rb"dim % 4 == 0, 4 <= dim <= 2048"),
        (lambda: lib.nd_layernorm_bwd(P, P, P, None, P, None, 4, 2052, 1e-6, None), rb"dim % 4 == 0, 4 <= dim <= 2048"),
        (lambda: lib.nd_layernorm_bwd(P, P, P, None, None, P, 4, 36, 1e-6, None), rb"split \(frag32b3\) output needs dim % 32 == 0"),
        (lambda: lib.nd_xent_head_bwd(P, P, P, P, P, 2, 1025, 768, None), rb"C <= 1024 \(C=1025\)"),
        (lambda: lib.nd_unpatchify(P, P, 2, 3, 24, 24, 6, None), rb"patch size must be a multiple of 4"),
        (lambda: lib.nd_linf_random_start(P, P, 2, 6, 1, 0, 0, 0.1, 0.0, 1.0, None), rb"per_image % 4 == 0"),
    ]
    for call, msg in cases:
        assert call() == -1, msg                                   # ND_ERR_ARG
        assert re.search(msg, lib.nd_last_error()), (msg, lib.nd_last_error())
