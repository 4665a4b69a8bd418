"""AutoAttack's APGD-CE on the GPU (nd_apgd_* in csrc/nd_attack_linf.hip, nested_diffusion_amd/autoattack.py): the random start and every
iteration's arrays bit for bit against a float32 restatement of autoattack's listing on the host, the gradients against float64 autograd
through the oracle, run_standard_evaluation's row rules, the attacked tree end to end, the production shape and the attack's strength."""
import os

import numpy as np
import pytest
import torch

from oracle import ref_cpu
from test_gpu_attack import TAU, f64, images, ref_grad, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
APGD_TAG = 0x41504731
F32 = torch.float32


@pytest.fixture(scope="module")
def tiny():
    from nested_diffusion_amd.mapping import VisionTransformer
    vp = ref_cpu.init_vit_params(embed=128, depth=5, patch=16, img=32, seed=3)
    return VisionTransformer(vp, 2, DEV), vp, 2, 5, 32


# ---- host float32 restatement ----------------------------------------------------------------------------------------------------
def host_random_start(x0, index, eps, seed, restart):
    """autoattack's x + eps * t / (max|t| + 1e-12), clamp(0, 1), with t = 2u - 1 from the Philox words (counter = (index, quad,
    restart, tag)); each operation one fp32 rounding."""
    x0 = x0.float().cpu()
    B, per = x0.shape[0], x0[0].numel()
    Q = per // 4
    b, q = np.meshgrid(np.asarray(index, dtype=np.int64), np.arange(Q), indexing="ij")
    ctr = np.stack([b & 0xFFFFFFFF, q, np.full_like(q, restart), np.full_like(q, APGD_TAG)], axis=-1).reshape(-1, 4)
    w = ref_cpu.philox4x32_10(ctr, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF).reshape(B, per)
    u = (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    t = np.float32(2.0) * u - np.float32(1.0)
    m = np.abs(t).max(axis=1, keepdims=True) + np.float32(1e-12)
    y = x0.numpy().reshape(B, per) + np.float32(eps) * (t / m)
    return torch.from_numpy(np.clip(y, np.float32(0.0), np.float32(1.0)).reshape(x0.shape))


class HostAPGD:
    """attack_single_run in float32 on the host, fed the GPU's logits, gradient and loss of each iteration."""

    def __init__(self, x, y, eps, n_iter, schedule, rho=0.75):
        self.x, self.y = x.float().cpu(), y.cpu()
        e = torch.tensor(eps, dtype=F32)
        self.lo, self.hi = self.x - e, self.x + e
        self.eps, self.n_iter, self.schedule, self.rho = e, n_iter, schedule, rho
        self.restores = self.keeps = 0

    def init(self, x_adv, logits, grad, loss):
        self.x_adv = x_adv.cpu().clone()
        self.acc = logits.cpu().argmax(1) == self.y
        self.loss_best = loss.cpu().clone()
        self.x_best, self.x_best_adv, self.grad_best, self.grad = self.x_adv.clone(), self.x_adv.clone(), grad.cpu().clone(), grad.cpu().clone()
        self.step = torch.full((x_adv.shape[0],), 2.0, dtype=F32) * self.eps
        self.x_adv_old = self.x_adv.clone()
        self.loss_best_last_check, self.reduced_last_check = self.loss_best.clone(), torch.ones_like(self.loss_best)
        self.loss_steps = torch.zeros(self.n_iter, x_adv.shape[0], dtype=F32)

    def do_step(self, i):
        a = 1.0 if i == 0 else 0.75
        grad2 = self.x_adv - self.x_adv_old
        self.x_adv_old = self.x_adv
        s = torch.nan_to_num(torch.sign(self.grad), nan=0.0)
        st = self.step.view(-1, 1, 1, 1)
        z = torch.clamp(torch.min(torch.max(self.x_adv + st * s, self.lo), self.hi), 0.0, 1.0)
        v = (self.x_adv + (z - self.x_adv) * a) + grad2 * (1 - a)
        self.x_adv = torch.clamp(torch.min(torch.max(v, self.lo), self.hi), 0.0, 1.0)

    def observe(self, i, logits, grad, loss):
        logits, grad, loss = logits.cpu(), grad.cpu().clone(), loss.cpu().clone()
        self.grad = grad
        pred = logits.argmax(1) == self.y
        self.acc = self.acc & pred
        self.x_best_adv[~pred] = self.x_adv[~pred]
        self.loss_steps[i] = loss
        imp = loss > self.loss_best
        self.x_best[imp], self.grad_best[imp], self.loss_best[imp] = self.x_adv[imp], grad[imp], loss[imp]
        k = self.schedule.get(i, 0)
        if k:
            cnt = torch.zeros_like(loss)
            for c in range(k):
                cnt += (self.loss_steps[i - c] > self.loss_steps[i - c - 1]).float()      # row -1: the last row, as torch indexes
            osc = (cnt <= k * self.rho) | ((self.reduced_last_check == 0) & (self.loss_best_last_check >= self.loss_best))
            self.reduced_last_check = osc.float()
            self.loss_best_last_check = self.loss_best.clone()
            self.step[osc] = self.step[osc] / 2.0
            self.x_adv[osc] = self.x_best[osc]
            self.grad[osc] = self.grad_best[osc]
            self.restores += int(osc.sum())
            self.keeps += int((~osc).sum())


def run_parity(vit, x, y, eps, n_iter, check_upto, seed=5, restart=0, grad_oracle=None):
    """attack_single_run on the GPU with every array compared bit for bit against HostAPGD up to iteration check_upto."""
    from nested_diffusion_amd.autoattack import APGDAttack
    atk = APGDAttack(vit, n_iter=n_iter, eps=eps, seed=seed)
    host = HostAPGD(x, y, eps, n_iter, atk.schedule)
    index = torch.arange(x.shape[0], device=DEV) + 100
    worst = [0.0, 0.0]

    def same(name, gpu, want, i):
        assert torch.equal(gpu.cpu(), want), (name, i, float((gpu.cpu().double() - want.double()).abs().max()))

    def trace(i, logits, grad, loss, arrays, st):
        if i > check_upto:
            return
        if grad_oracle is not None:                             # the gradient at this iteration's input point
            r, m = grad_oracle(arrays["x_adv"].cpu() if i < 0 else host.x_adv, grad)
            worst[0], worst[1] = max(worst[0], r), max(worst[1], m)
        if i < 0:
            same("start", arrays["x_adv"], host_random_start(x, index.cpu().numpy(), eps, seed, restart), i)
            host.init(arrays["x_adv"], logits, grad, loss)
        else:
            host.observe(i, logits, grad, loss)
            if i + 1 < n_iter:
                host.do_step(i + 1)
        if i < 0:
            host.do_step(0)
            return                                              # the first step runs after this call
        same("x_adv", arrays["x_adv"], host.x_adv, i)
        if i + 1 < n_iter:
            same("x_adv_old", arrays["x_adv_old"], host.x_adv_old, i)
        for name in ("x_best", "grad_best", "x_best_adv"):
            same(name, arrays[name], getattr(host, name), i)
        same("step", st.step, host.step, i)
        same("loss_best", st.loss_best, host.loss_best, i)
        same("acc", st.acc.bool(), host.acc, i)

    acc, adv = atk.attack_single_run(x.to(DEV), y.to(DEV), index, restart=restart, trace=trace)
    return host, acc, adv, worst


# ---- 1. random start -------------------------------------------------------------------------------------------------------------
def test_random_start_bitwise_and_keyed_on_the_global_index():
    from nested_diffusion_amd import ops
    x = images(4, 32, 61)
    eps, seed = 8 / 255, 0x0123_4567_89AB_CDEF
    idx = torch.tensor([10, 11, 12, 13])
    s = ops.apgd_random_start(x.to(DEV), idx.to(DEV), eps, seed, restart=2)
    assert torch.equal(s.cpu(), host_random_start(x, idx.numpy(), eps, seed, 2))
    sub = ops.apgd_random_start(x[[1, 3]].to(DEV), idx[[1, 3]].to(DEV), eps, seed, restart=2)   # a compacted restart subset
    assert torch.equal(sub, s[[1, 3]])
    assert float((s.cpu() - x).abs().max()) <= eps * (1 + 1e-6)
    assert float(s.min()) >= 0 and float(s.max()) <= 1
    other = ops.apgd_random_start(x.to(DEV), idx.to(DEV), eps, seed, restart=3)
    assert not torch.equal(other, s)
    # each row's draw reaches the box's face in some element: the normalisation by max|t| (within the [0, 1] clamp)
    d = (s.cpu() - x).abs().flatten(1).max(1).values
    assert float(d.min()) >= eps * 0.99
    # the PGD start draws with another tag: an independent start
    assert not torch.equal(ops.linf_random_start(x.to(DEV), eps, seed, 10, 2), s)


def test_random_start_at_production_shape():
    from nested_diffusion_amd import ops
    x = images(3, 224, 62)
    idx = torch.tensor([7, 0, 2 ** 32 + 5])                   # the counter takes the index's low word
    s = ops.apgd_random_start(x.to(DEV), idx.to(DEV), 4 / 255, 9, restart=0)
    assert torch.equal(s.cpu(), host_random_start(x, idx.numpy(), 4 / 255, 9, 0))


# ---- 2. loop parity ------------------------------------------------------------------------------------------------------------------
def test_loop_parity_tiny_vit_full_run(tiny):
    vit, vp, heads, depth, img = tiny
    vp64 = f64(vp)
    x = images(8, img, 71)
    y = torch.tensor([0, 1, 1, 0, 1, 0, 0, 1])

    def oracle(x_in, grad):
        _, g_ref = ref_grad(vp64, x_in, y, heads, depth)
        return rel_l2(grad, g_ref), float((grad.cpu().double() - g_ref).abs().max() / g_ref.abs().max())

    host, acc, adv, worst = run_parity(vit, x, y, 8 / 255, 100, 100, grad_oracle=oracle)
    print(f"apgd tiny B=8: {host.restores} restores, {host.keeps} kept checkpoints; gradient rel L2 <= {worst[0]:.2e}, max <= {worst[1]:.2e}")
    assert host.restores >= 1 and host.keeps >= 1               # both branches of the checkpoint rule ran
    assert worst[0] <= 1e-4 and worst[1] <= TAU
    assert torch.equal(acc.cpu(), host.acc)
    assert torch.equal(adv.cpu(), host.x_best_adv)


# ---- 3. run_standard_evaluation ---------------------------------------------------------------------------------------------------------
def _aa(vit, eps, **kw):
    from nested_diffusion_amd.autoattack import AutoAttack
    return AutoAttack(vit, eps=eps, version="custom", norm="Linf", attacks_to_run=["apgd-ce"], **kw)


def _check_rows(vit, x, y, adv, eps, clean_wrong):
    """The row rules of run_standard_evaluation; returns the changed rows."""
    x, adv = x.cpu(), adv.cpu()
    pred = vit.forward(adv.to(DEV)).argmax(1).cpu()
    changed = (adv != x).flatten(1).any(1)
    assert not changed[clean_wrong].any()                       # misclassified at the start: unchanged
    assert not changed[pred == y].any()                         # never fooled: unchanged (bit for bit)
    assert bool((pred[changed] != y[changed]).all())            # every changed row is misclassified by forward
    assert float((adv - x).abs().max()) <= eps * (1 + 1e-6)
    assert float(adv.min()) >= 0 and float(adv.max()) <= 1
    return changed


def test_run_standard_evaluation_rows_and_restarts(tiny):
    vit = tiny[0]
    x = images(32, 32, 101)                                     # the strength test's batch: at 8/255 some rows are fooled, some not
    clean = vit.forward(x.to(DEV)).argmax(1).cpu()
    y = clean.clone()
    flip = torch.tensor([2, 5, 17, 30])
    y[flip] = 1 - y[flip]                                       # misclassified from the start
    eps = 8 / 255
    aa = _aa(vit, eps, seed=1)
    sizes = []
    orig = vit.input_grad

    def counting(xx, yy):
        sizes.append(xx.shape[0])
        return orig(xx, yy)

    vit.input_grad = counting
    try:
        adv = aa.run_standard_evaluation(x.to(DEV), y.to(DEV), bs=32, first_image=0)
    finally:
        del vit.input_grad
    changed = _check_rows(vit, x, y, adv, eps, clean != y)
    robust = 32 - len(flip)
    assert 0 < int(changed.sum()) < robust                      # both kinds of row occur
    # restarts re-attack only the survivors: runs of 101 gradients whose batch never grows, down to the rows never fooled
    assert len(sizes) == 5 * 101
    runs = [sizes[r * 101:(r + 1) * 101] for r in range(5)]
    assert all(len(set(r)) == 1 for r in runs)
    n = [r[0] for r in runs]
    assert n[0] == robust and all(a >= b for a, b in zip(n, n[1:])) and n[-1] >= robust - int(changed.sum())
    print(f"apgd rows: restart batch sizes {n}, {int(changed.sum())} of {robust} fooled")
    # the keyed start: the same call again gives the same bits
    assert torch.equal(aa.run_standard_evaluation(x.to(DEV), y.to(DEV), bs=32), adv)


# ---- 4. apply_attack / test_atk / make_attacks AUTOPGD --------------------------------------------------------------------------------
def test_make_attacks_autopgd_and_the_attacked_dataset(tmp_path, capsys, monkeypatch):
    from test_gpu_attack_e2e import EPS, FLAGS, _reload_png, _run_main
    from test_gpu_cli import _write_image_tree, _write_run
    import yaml
    import nested_diffusion_amd.runner as runner_mod
    from nested_diffusion_amd import make_attacks
    from nested_diffusion_amd.attack import apply_attack
    from nested_diffusion_amd.autoattack import AutoAttack
    from nested_diffusion_amd.data import ImageFolderDataset
    tmp = str(tmp_path)
    ypath, *_ = _write_run(tmp, T=6, K=5, B=3, img=224)
    dataroot = os.path.join(tmp, "data")
    _write_image_tree(dataroot)
    out = os.path.join(tmp, "attacked")
    assert make_attacks.main(["--config", ypath, "--attack_name", "AUTOPGD", "--eps", str(EPS), "--out", out, "--dataroot", dataroot,
                              "--batch_size", "3", "--seed", "2"]) == 0
    assert "AUTOPGD eps=" in capsys.readouterr().out
    tree = os.path.join(out, "Test_attacks_AUTOPGD")
    assert sorted(os.listdir(tree)) == ["NORMAL", "PNEUMONIA"]
    clean = ImageFolderDataset(os.path.join(dataroot, "testing"), "ChestXRay", "grayscaled")
    for path, t in clean.samples:
        cls = os.path.basename(os.path.dirname(path))
        adv = _reload_png(os.path.join(tree, cls, os.path.splitext(os.path.basename(path))[0] + ".png"))
        x, _ = clean[clean.samples.index((path, t))]
        assert float((adv - x).abs().max()) <= EPS + 0.5 / 255 + 1e-6
    # main.py --test evaluates the tree through the ChestXRayAtkAUTOPGD dataset name
    cfg = yaml.safe_load(open(ypath))
    cfg["data"]["dataset"], cfg["data"]["dataroot"] = "ChestXRayAtkAUTOPGD", out
    y2 = os.path.join(tmp, "atk.yml")
    yaml.safe_dump(cfg, open(y2, "w"))
    assert _run_main(FLAGS + ["--config", y2, "--doc", "apgd", "--exp", os.path.join(tmp, "r1")]) == 0
    assert "Majority voting accuracy for MC:" in capsys.readouterr().out
    # test_atk(attack=AutoAttack(...)) equals test_atk on apply_attack's output
    items = [clean[i] for i in range(6)]
    batches = [(torch.stack([x for x, _ in items[k:k + 3]]), torch.tensor([t for _, t in items[k:k + 3]])) for k in (0, 3)]
    reports = {}
    orig_atk = runner_mod.Diffusion.test_atk

    def spy(self, test_loader=None, attack=None):
        atk = AutoAttack(self.cond_pred_model, eps=EPS, seed=3, version="custom", norm="Linf", attacks_to_run=["apgd-ce"])
        atk.apgd.n_restarts = 2
        orig_atk(self, test_loader=batches, attack=atk)
        reports["atk"] = self.last_report
        adv = [(apply_attack(atk, x.to(self.device), t.to(self.device), "AUTOPGD", first_image=3 * n).cpu(), t)
               for n, (x, t) in enumerate(batches)]
        orig_atk(self, test_loader=adv)
        reports["apply"] = self.last_report
        return orig_atk(self, test_loader=batches)

    monkeypatch.setattr(runner_mod.Diffusion, "test_atk", spy)
    assert _run_main(FLAGS + ["--config", ypath, "--dataroot", dataroot, "--doc", "apgd3", "--exp", os.path.join(tmp, "r3")]) == 0
    for k in reports["atk"]:
        ta, tb = torch.as_tensor(reports["atk"][k]), torch.as_tensor(reports["apply"][k])
        assert torch.allclose(ta, tb, rtol=0, atol=0, equal_nan=True), k


# ---- 5. production shape ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vitb():
    from nested_diffusion_amd.mapping import VisionTransformer
    vp = ref_cpu.init_vit_params(embed=768, depth=12, patch=16, img=224, seed=11)
    return VisionTransformer(vp, 12, DEV)


def test_production_shape_parity_and_rows(vitb):
    x = images(32, 224, 91)
    y = torch.arange(32) % 2
    host, acc, adv, _ = run_parity(vitb, x, y, 8 / 255, 100, 24)          # iterations 0..24: through the first checkpoint (i = 21)
    clean = vitb.forward(x.to(DEV)).argmax(1).cpu()
    aa = _aa(vitb, 1 / 255)
    aa.apgd.n_restarts = 1
    out = aa.run_standard_evaluation(x.to(DEV), y.to(DEV), bs=32)
    changed = _check_rows(vitb, x, y, out, 1 / 255, clean != y)
    assert 0 < int(changed.sum()) < int((clean == y).sum())      # both kinds of row occur
    print(f"apgd ViT-B/16 B=32: {int(changed.sum())} of {int((clean == y).sum())} fooled in one restart")


# ---- 6. strength -----------------------------------------------------------------------------------------------------------------------
def test_apgd_fools_at_least_as_many_as_pgd(tiny):
    from nested_diffusion_amd.attack import Attack
    vit = tiny[0]
    eps = 8 / 255
    x = images(32, 32, 101).to(DEV)
    y = vit.forward(x).argmax(1)                                # every image starts correctly classified
    _, pgd_ok = Attack(eps, "PGD", vit, seed=1).generate_attack(x, y)
    adv = _aa(vit, eps, seed=1).run_standard_evaluation(x, y, bs=32)
    apgd_ok = vit.forward(adv).argmax(1) != y
    print(f"eps 8/255, 32 images: PGD fools {int(pgd_ok.sum())}, APGD {int(apgd_ok.sum())}")
    assert int(apgd_ok.sum()) >= int(pgd_ok.sum())
