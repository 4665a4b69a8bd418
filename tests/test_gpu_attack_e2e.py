"""Attacked test sets end to end on the GPU: make_attacks writes the Test_attacks_<NAME> tree, main.py --test evaluates it through the
ChestXRayAtk* dataset name, and test_atk(attack=...) equals test_atk on apply_attack's output."""
import os

import numpy as np
import pytest
import torch
import yaml

from test_gpu_cli import _write_image_tree, _write_run

pytestmark = pytest.mark.gpu
EPS = 8 / 255
FLAGS = ["--test", "--device", "0", "--thread", "8", "--loss", "card_onehot_conditional", "--n_splits", "1", "--noise_perturbation", "0",
         "--low_resolution", "0", "--brightness", "0", "--contrast", "1", "--crop", "0", "--attack_name", "None", "--eps", "0", "--ni",
         "--preprocess", "grayscaled", "--timesteps", "6", "--seed", "7", "--mc_trials", "2"]


def _reload_png(path):
    from PIL import Image
    return torch.from_numpy(np.array(Image.open(path).convert("RGB"), dtype=np.uint8)).permute(2, 0, 1).float().div(255)


@pytest.fixture(scope="module")
def attacked(tmp_path_factory):
    from nested_diffusion_amd import make_attacks
    tmp = str(tmp_path_factory.mktemp("atk"))
    ypath, *_ = _write_run(tmp, T=6, K=5, B=3, img=224)
    dataroot = os.path.join(tmp, "data")
    _write_image_tree(dataroot)
    out = os.path.join(tmp, "attacked")
    assert make_attacks.main(["--config", ypath, "--attack_name", "FGSM", "--eps", str(EPS), "--out", out, "--dataroot", dataroot,
                              "--batch_size", "3"]) == 0
    return tmp, ypath, dataroot, out


def test_make_attacks_writes_the_tree(attacked):
    from nested_diffusion_amd.data import ImageFolderDataset
    tmp, ypath, dataroot, out = attacked
    tree = os.path.join(out, "Test_attacks_FGSM")
    assert sorted(os.listdir(tree)) == ["NORMAL", "PNEUMONIA"]
    assert sorted(os.listdir(os.path.join(tree, "NORMAL"))) == ["a_same.png", "b_gray.png", "c_big.png", "d_wide.png"]
    assert sorted(os.listdir(os.path.join(tree, "PNEUMONIA"))) == ["e_tall.png", "f_gray_small.png", "g_last.png"]
    clean = ImageFolderDataset(os.path.join(dataroot, "testing"), "ChestXRay", "grayscaled")
    for path, _ in clean.samples:
        cls = os.path.basename(os.path.dirname(path))
        stem = os.path.splitext(os.path.basename(path))[0]
        adv = _reload_png(os.path.join(tree, cls, stem + ".png"))
        x, _ = clean[clean.samples.index((path, clean.class_to_idx[cls]))]
        assert float((adv - x).abs().max()) <= EPS + 0.5 / 255 + 1e-6


def _run_main(argv):
    from nested_diffusion_amd import main as nd_main
    import nested_diffusion_amd.mapping as mapping
    import nested_diffusion_amd.runner as runner_mod
    orig = mapping.load_conditioner
    # the tiny ViT of these checkpoints has 2 heads of 64: the loader's default is 12
    patched = lambda path, ds, device="cuda", num_heads=12, dtype="f32": orig(path, ds, device, 2, dtype)   # noqa: E731
    runner_mod.load_conditioner = patched
    try:
        return nd_main.main(argv)
    finally:
        runner_mod.load_conditioner = orig


def test_main_evaluates_the_attacked_dataset(attacked, capsys, monkeypatch):
    import nested_diffusion_amd.runner as runner_mod
    tmp, ypath, dataroot, out = attacked
    cfg = yaml.safe_load(open(ypath))
    cfg["data"]["dataset"] = "ChestXRayAtkFGSM"
    cfg["data"]["dataroot"] = out
    y2 = os.path.join(tmp, "chest_x_ray_atk.yml")
    yaml.safe_dump(cfg, open(y2, "w"))
    assert _run_main(FLAGS + ["--config", y2, "--doc", "atk", "--exp", os.path.join(tmp, "r1")]) == 0
    rep1 = capsys.readouterr().out
    assert "Majority voting accuracy for MC:" in rep1
    # the same report from test_atk on the PNGs reloaded here (ImageFolder order: classes sorted, files sorted; batch 3, drop_last)
    tree = os.path.join(out, "Test_attacks_FGSM")
    files = [(os.path.join(tree, c, f), i) for i, c in enumerate(sorted(os.listdir(tree))) for f in sorted(os.listdir(os.path.join(tree, c)))]
    batches = [(torch.stack([_reload_png(p) for p, _ in files[k:k + 3]]), torch.tensor([t for _, t in files[k:k + 3]]))
               for k in range(0, len(files) - 2, 3)]
    orig_atk = runner_mod.Diffusion.test_atk
    monkeypatch.setattr(runner_mod.Diffusion, "test_atk", lambda self, test_loader=None, attack=None: orig_atk(self, test_loader=batches))
    assert _run_main(FLAGS + ["--config", y2, "--doc", "atk2", "--exp", os.path.join(tmp, "r2")]) == 0
    rep2 = capsys.readouterr().out
    key = lambda s: [l for l in s.splitlines() if l.startswith(("Majority", "ECE", "Average"))]   # noqa: E731
    assert key(rep1) == key(rep2) and len(key(rep1)) == 6


def test_test_atk_with_an_attack_equals_apply_attack(attacked, monkeypatch, capsys):
    import nested_diffusion_amd.runner as runner_mod
    from nested_diffusion_amd.attack import Attack, apply_attack
    from nested_diffusion_amd.data import ImageFolderDataset
    tmp, ypath, dataroot, out = attacked
    clean = ImageFolderDataset(os.path.join(dataroot, "testing"), "ChestXRay", "grayscaled")
    items = [clean[i] for i in range(6)]
    batches = [(torch.stack([x for x, _ in items[k:k + 3]]), torch.tensor([t for _, t in items[k:k + 3]])) for k in (0, 3)]
    reports = {}
    orig_atk = runner_mod.Diffusion.test_atk

    def spy(self, test_loader=None, attack=None):
        for kind in ("PGD", "FGSM"):
            atk = Attack(EPS, kind, self.cond_pred_model, seed=3)
            orig_atk(self, test_loader=batches, attack=atk)
            reports[kind] = self.last_report
            adv = [(apply_attack(atk, x.to(self.device), t.to(self.device), kind, first_image=3 * n).cpu(), t)
                   for n, (x, t) in enumerate(batches)]
            orig_atk(self, test_loader=adv)
            reports[kind + "_apply"] = self.last_report
        return orig_atk(self, test_loader=batches)

    monkeypatch.setattr(runner_mod.Diffusion, "test_atk", spy)
    assert _run_main(FLAGS + ["--config", ypath, "--dataroot", dataroot, "--doc", "atk3", "--exp", os.path.join(tmp, "r3")]) == 0
    for kind in ("PGD", "FGSM"):
        a, b = reports[kind], reports[kind + "_apply"]
        for k in a:
            ta, tb = torch.as_tensor(a[k]), torch.as_tensor(b[k])
            assert torch.allclose(ta, tb, rtol=0, atol=0, equal_nan=True), (kind, k)      # bitwise; a class without votes is NaN
