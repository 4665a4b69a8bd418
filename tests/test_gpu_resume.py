"""Resumable training on the GPU: for each of the three trainers a 4-epoch run straight through (A), the same run with a snapshot after
every epoch (B), and the run cut after 2 epochs, everything rebuilt from scratch with every generator disturbed, and resumed for 2 more
(C) end in the same bits -- every tensor and counter of training_state(), the loop's results and the best checkpoint file.  Then the
pieces on their own: the in-library sampler state read and restored (EnsembleEngine.rng_state / set_rng_state), and
load_training_state(training_state()) on the raw packed / frag32b3 images.

Every comparison is bit for bit, so there is no tolerance to choose.  The shapes are the smallest that keep every edge: lin1.lin.weight
with 4 real columns of 16, a last training batch shorter than the others, packed images with 3 real rows of 16.  The noise estimator's
conditioner is a frozen stand-in (a fixed matrix per mapping MLP): at data_dim 48 the images are 4 x 4, no size a ViT of this package
is built for, and a conditioner holds nothing a snapshot carries -- it is neither trained nor does it draw."""
import argparse
import os
import shutil

import pytest
import torch

from oracle import ref_cpu
from test_gpu_diffusion_train import config_of

pytestmark = pytest.mark.gpu
DEV = "cuda"
ns = argparse.Namespace


class Preempted(Exception):
    """what stands for the interruption of a run: raised by the training loader at the top of an epoch"""


class StoppingLoader(torch.utils.data.DataLoader):
    """a DataLoader that raises Preempted instead of starting its (stop_after + 1)-th pass"""

    def __init__(self, *a, stop_after=None, **kw):
        super().__init__(*a, **kw)
        self.passes, self.stop_after = 0, stop_after

    def __iter__(self):
        if self.passes == self.stop_after:
            raise Preempted()
        self.passes += 1
        return super().__iter__()


def loaders(x, y, xv, yv, batch, valid_batch, seed, stop_after=None):
    """(training loader, shuffled under its own generator; validation loader in order)"""
    g = torch.Generator().manual_seed(seed)
    train = StoppingLoader(torch.utils.data.TensorDataset(x, y), batch_size=batch, shuffle=True, generator=g, stop_after=stop_after)
    return train, torch.utils.data.DataLoader(torch.utils.data.TensorDataset(xv, yv), batch_size=valid_batch, shuffle=False)


def disturb(train_loader):
    """every generator a loop draws from, moved on purpose before a resume"""
    torch.manual_seed(12345)
    torch.rand(3)
    torch.rand(3, device=DEV)
    torch.rand(1, generator=train_loader.generator)


def flat(state, pre=""):
    """a nested training state as {dotted key: leaf}"""
    out = {}
    for k, v in state.items():
        if isinstance(v, dict):
            out.update(flat(v, f"{pre}{k}/"))
        else:
            out[f"{pre}{k}"] = v
    return out


def same_state(a, b, skip=("meta/epochs",)):
    """every tensor torch.equal (and of one dtype and shape), every counter and field equal; returns the number of tensors compared"""
    fa, fb = flat(a), flat(b)
    assert sorted(fa) == sorted(fb)
    n = 0
    for k in fa:
        if k in skip:
            continue
        if torch.is_tensor(fa[k]):
            assert fa[k].dtype == fb[k].dtype and fa[k].device.type == "cpu" and torch.equal(fa[k], fb[k]), k
            n += 1
        else:
            assert fa[k] == fb[k], (k, fa[k], fb[k])
    return n


def differs(a, b):
    fa, fb = flat(a), flat(b)
    return any(not torch.equal(fa[k], fb[k]) for k in fa if torch.is_tensor(fa[k]))


def same_file(pa, pb):
    a, b = flat(torch.load(pa)), flat(torch.load(pb))
    assert sorted(a) == sorted(b) and a
    for k in a:
        assert (torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k]), k


# ---- 1. the noise estimator: Diffusion.train ----------------------------------------------------------------------------------------------
NE = dict(B=6, D=48, H=32, F=32, C=2, T=6, K=2, n_train=16, n_valid=8, valid_batch=4, epochs=4, mlp_idx=1)


class FrozenConditioner:
    """compute_guiding_prediction of K mapping MLPs as K fixed matrices on the flattened image (see the module docstring)"""

    def __init__(self, K, D, C, seed):
        g = torch.Generator().manual_seed(seed)
        self.mlps = [None] * K
        self.w = [torch.randn(D, C, generator=g).to(DEV) for _ in range(K)]

    def compute_guiding_prediction(self, x, include_full_vit=True):
        f = torch.flatten(x.to(DEV, torch.float32), 1)
        out = [f @ w for w in self.w]
        return out + [out[-1].clone()] if include_full_vit else out


def noise_data():
    g = torch.Generator().manual_seed(21)
    c = NE
    side = 4                                                     # 3 x 4 x 4 = data_dim 48
    return (torch.rand(c["n_train"], 3, side, side, generator=g), torch.randint(0, c["C"], (c["n_train"],), generator=g),
            torch.rand(c["n_valid"], 3, side, side, generator=g), torch.randint(0, c["C"], (c["n_valid"],), generator=g))


def noise_run(log_dir, snapshot_epochs=None, resume=False, stop_after=None):
    """One Diffusion.train from scratch objects: (the returned dict or None if the run was cut, the runner)."""
    from nested_diffusion_amd.runner import Diffusion
    c = NE
    os.makedirs(log_dir, exist_ok=True)
    cfg = config_of(c["B"], c["D"], c["H"], c["F"], c["C"], c["T"])
    cfg.training.n_epochs, cfg.testing.batch_size = c["epochs"], c["valid_batch"]
    assert cfg.training.validation_freq == 1 and cfg.optim.lr_schedule and cfg.training.warmup_epochs == 1
    args = ns(seed=7, mc_trials=2, log_path=log_dir, preprocess="grayscaled", resume_training=resume)
    if snapshot_epochs is not None:
        args.snapshot_epochs = snapshot_epochs
    runner = Diffusion(args, cfg, device=DEV, conditioner=FrozenConditioner(c["K"], c["D"], c["C"], seed=3))
    train, valid = loaders(*noise_data(), c["B"], c["valid_batch"], seed=5, stop_after=stop_after)
    assert len(train) == 3 and c["n_train"] % c["B"] == 4        # the last batch has 4 rows
    if resume:
        disturb(train)
    try:
        return runner.train(c["mlp_idx"], train_loader=train, valid_loader=valid), runner
    except Preempted:
        return None, runner


@pytest.fixture(scope="module")
def noise_runs(tmp_path_factory):
    """A once, and the first half of C once (its log folder is copied by every test that resumes from it)."""
    root = tmp_path_factory.mktemp("noise")
    res_a, run_a = noise_run(str(root / "A"))
    assert not os.path.exists(str(root / "A" / "ckpt.pth"))      # no flag, no snapshot
    half, run_h = noise_run(str(root / "half"), snapshot_epochs=1, stop_after=2)
    assert half is None and run_h.trainer.t == 6 and os.path.exists(str(root / "half" / "ckpt.pth"))
    return {"root": root, "A": res_a, "state_A": run_a.trainer.training_state()}


def check_noise_against_a(runs, res, runner):
    a = runs["A"]
    assert res["losses"] == a["losses"] and len(res["losses"]) == NE["epochs"]
    assert res["accuracies"] == a["accuracies"] and sorted(res["accuracies"]) == list(range(NE["epochs"]))
    assert a["best"] is not None and os.path.basename(res["best"]) == os.path.basename(a["best"])
    same_file(res["best"], a["best"])
    n = same_state(runner.trainer.training_state(), runs["state_A"])
    assert n == 3 * 29 + 12                                      # p, m, v of the 29 parameters, six running means and variances
    assert runner.trainer.t == 12 and runner.trainer.batches_tracked == 12


def test_noise_estimator_straight_snapshotting_and_resumed_runs_end_in_the_same_bits(noise_runs):
    root = noise_runs["root"]
    st = noise_runs["state_A"]
    assert tuple(st["p"]["lin1.lin.weight"].shape) == tuple(st["m"]["lin1.lin.weight"].shape) == (NE["F"], 2 * NE["C"])
    assert st["t"] == 12 and st["meta"]["kind"] == "noise_estimator" and st["meta"]["train_batches"] == 3 and st["meta"]["batch_size"] == 6
    assert float(st["m"]["encoder_x.0.weight"].abs().max()) > 0 and float(st["v"]["lin4.weight"].abs().max()) > 0
    # B: a snapshot after every epoch changes nothing
    res_b, run_b = noise_run(str(root / "B"), snapshot_epochs=1)
    check_noise_against_a(noise_runs, res_b, run_b)
    snap = torch.load(str(root / "B" / "ckpt.pth"))
    assert sorted(snap) == ["loop", "rng", "trainer"] and snap["loop"]["next_epoch"] == 4 and snap["loop"]["step"] == 12
    assert sorted(snap["loop"]) == ["accuracies", "best", "losses", "max_accuracy", "next_epoch", "step"]
    assert sorted(snap["rng"]) == ["cpu", "cuda", "engine", "loader"] and len(snap["rng"]["engine"]) == 2 and snap["rng"]["loader"] is not None
    assert same_state(snap["trainer"], noise_runs["state_A"]) == 3 * 29 + 12
    assert not os.path.exists(str(root / "B" / "ckpt.pth.tmp"))
    # C: cut after two epochs, everything rebuilt, every generator disturbed, resumed
    shutil.copytree(str(root / "half"), str(root / "C"))
    half = torch.load(str(root / "C" / "ckpt.pth"))
    assert half["loop"]["next_epoch"] == 2 and half["loop"]["step"] == 6 and half["trainer"]["t"] == 6
    res_c, run_c = noise_run(str(root / "C"), snapshot_epochs=1, resume=True)
    check_noise_against_a(noise_runs, res_c, run_c)
    assert torch.load(str(root / "C" / "ckpt.pth"))["loop"]["next_epoch"] == 4
    # the best file keeps its layout
    ck = torch.load(res_c["best"])
    assert set(ck) == {"noise_estimator", "optimizer", "epoch"} and set(ck["optimizer"]) == {"step", "lr"}


def _tamper(snap, what):
    if what in ("cpu", "cuda", "loader"):
        cur = {"cpu": torch.get_rng_state(), "cuda": torch.cuda.get_rng_state(DEV), "loader": torch.Generator().manual_seed(99).get_state()}
        assert not torch.equal(snap["rng"][what], cur[what])
        snap["rng"][what] = cur[what]
    elif what == "t":
        snap["trainer"]["t"] += 1
    elif what == "next_epoch":                                   # the lr_at epoch index: the same two epochs, one index early
        snap["loop"]["next_epoch"] -= 1
    elif what == "batches_tracked":
        snap["trainer"]["batches_tracked"] += 1
    else:
        snap["trainer"][what]["lin2.lin.weight"].zero_()


@pytest.mark.parametrize("what", ["cpu", "cuda", "loader", "t", "m", "v", "next_epoch", "batches_tracked"])
def test_a_resume_that_misses_one_piece_of_state_ends_elsewhere(noise_runs, what):
    """The control of the test above: with one stream, counter or moment of the snapshot replaced, the resumed run no longer ends in A's
    bits -- so agreement there shows that each of them was restored."""
    root = noise_runs["root"]
    log_dir = str(root / f"miss_{what}")
    shutil.copytree(str(root / "half"), log_dir)
    snap = torch.load(os.path.join(log_dir, "ckpt.pth"))
    torch.manual_seed(4321)
    _tamper(snap, what)
    torch.save(snap, os.path.join(log_dir, "ckpt.pth"))
    _, run = noise_run(log_dir, resume=True, stop_after=2)       # two more epochs, then cut: epochs 2, 3 (or 1, 2 for next_epoch)
    got = run.trainer.training_state()
    if what == "batches_tracked":
        assert got["batches_tracked"] == 13 and noise_runs["state_A"]["batches_tracked"] == 12
    else:
        assert differs(got, noise_runs["state_A"])


def test_resume_refuses_another_member_or_loader_by_name(noise_runs):
    from nested_diffusion_amd.train_diffusion import NoiseEstimatorTrainer
    c = NE
    snap = torch.load(str(noise_runs["root"] / "half" / "ckpt.pth"))
    tr = NoiseEstimatorTrainer(config_of(c["B"], c["D"], c["H"], c["F"], c["C"], c["T"]), DEV, seed=1)
    meta = snap["trainer"]["meta"]
    for field, other in (("mlp_idx", 0), ("train_batches", 4), ("batch_size", 5)):
        tr.run_meta = {k: meta[k] for k in ("mlp_idx", "dataset", "train_batches", "batch_size", "epochs")}
        tr.run_meta[field] = other
        with pytest.raises(ValueError, match=rf"^{field}:"):
            tr.load_training_state(snap["trainer"])
    assert tr.t == 0
    other_dims = NoiseEstimatorTrainer(config_of(c["B"], c["D"], 48, c["F"], c["C"], c["T"]), DEV, seed=1)
    with pytest.raises(ValueError, match=r"^hidden_dim:"):
        other_dims.load_training_state(snap["trainer"])
    tr.run_meta = dict({k: meta[k] for k in ("mlp_idx", "dataset", "train_batches", "batch_size")}, epochs=400)   # a longer run is accepted
    tr.load_training_state(snap["trainer"])
    assert tr.t == 6 and tr.batches_tracked == 6


# ---- 2. the mapping MLP and the ViT: EpochTrainer._fit ------------------------------------------------------------------------------------
IMG = 32


@pytest.fixture(scope="module")
def frozen_vit():
    from nested_diffusion_amd.mapping import VisionTransformer
    return VisionTransformer(ref_cpu.init_vit_params(embed=128, depth=3, patch=16, img=IMG, num_classes=3, seed=3), 2, DEV)


def image_data(n_train, n_valid, classes, img, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n_train, 3, img, img, generator=g), torch.randint(0, classes, (n_train,), generator=g),
            torch.rand(n_valid, 3, img, img, generator=g), torch.randint(0, classes, (n_valid,), generator=g))


def mapping_run(vit, out_dir, epochs, **kw):
    from nested_diffusion_amd.train_mapping import MappingTrainer
    tr = MappingTrainer(vit, 1, num_classes=3, lr=1e-2, step_size=1, gamma=0.5, seed=0, in_features=(IMG // 16) ** 2 * 128, hidden=(48, 32, 16))
    assert tr.model.p["linear4.weight"].N == 3 and tr.model.p["linear1.weight"].N == 48
    train, valid = loaders(*image_data(16, 8, 3, IMG, seed=31), 6, 4, seed=5)
    if kw.get("resume"):
        disturb(train)
    return tr.fit(train, valid, epochs, out_dir, dataset="ChestXRay", **kw), tr


def vit_run(_, out_dir, epochs, **kw):
    from nested_diffusion_amd.train_transformer import ViTTrainer
    vp = ref_cpu.init_vit_params(embed=128, depth=1, patch=16, img=16, seed=43)
    tr = ViTTrainer(vp, num_classes=2, num_heads=2, lr=1e-3, step_size=1, gamma=0.5)
    train, valid = loaders(*image_data(8, 4, 2, 16, seed=32), 3, 2, seed=6)
    if kw.get("resume"):
        disturb(train)
    return tr.fit(train, valid, epochs, out_dir, "ChestXRay", **kw), tr


@pytest.mark.parametrize("kind", ["mapping", "vit"])
def test_fit_straight_snapshotting_and_resumed_runs_end_in_the_same_bits(kind, frozen_vit, tmp_path, capsys):
    run = {"mapping": mapping_run, "vit": vit_run}[kind]
    ckpt = {"mapping": os.path.join("MLPs", "block_1.ckpt"), "vit": "vit_base_patch16_224_ChestXRay.ckpt"}[kind]
    n_batches = {"mapping": 3, "vit": 3}[kind]
    d = {v: str(tmp_path / v) for v in "ABC"}
    hist_a, tr_a = run(frozen_vit, d["A"], 4)
    state_a = tr_a.training_state()
    assert not os.path.exists(os.path.join(d["A"], ckpt))
    assert state_a["t"] == 4 * n_batches and state_a["epoch"] == 4 and state_a["meta"]["kind"] == kind
    assert all(float(t.abs().max()) > 0 for which in "mv" for t in state_a[which].values())
    hist_b, tr_b = run(frozen_vit, d["B"], 4, snapshot_epochs=1)
    # C: two epochs, then a new trainer and new loaders with every generator disturbed, resumed for two more (the epoch count grows)
    hist_h, tr_h = run(frozen_vit, d["C"], 2, snapshot_epochs=1)
    half = torch.load(os.path.join(d["C"], ckpt))
    assert half["loop"]["next_epoch"] == 2 and half["trainer"]["t"] == 2 * n_batches and half["trainer"]["epoch"] == 2
    assert sorted(half["loop"]) == ["best_acc", "best_train_acc", "next_epoch", "saved_epochs"]
    assert sorted(half["rng"]) == ["cpu", "cuda", "engine", "loader"] and half["rng"]["engine"] is None and half["rng"]["loader"] is not None
    del tr_h
    hist_c, tr_c = run(frozen_vit, d["C"], 4, snapshot_epochs=1, resume=True)
    assert "Resumed from" in capsys.readouterr().out
    n_tensors = 3 * len(state_a["p"])
    for hist, tr, where in ((hist_b, tr_b, d["B"]), (hist_c, tr_c, d["C"])):
        for k in ("best_acc", "best_train_acc", "saved_epochs"):
            assert hist[k] == hist_a[k], (k, hist[k], hist_a[k])
        assert hist_a["saved_epochs"] and os.path.relpath(hist["path"], where) == os.path.relpath(hist_a["path"], d["A"])
        same_file(hist["path"], hist_a["path"])
        assert same_state(tr.training_state(), state_a) == n_tensors
        assert same_state(torch.load(os.path.join(where, ckpt))["trainer"], state_a) == n_tensors
        assert tr.lr == tr_a.lr == tr_a.base_lr / 16
    # without the loader generator's state the resumed run shuffles differently and ends elsewhere
    shutil.rmtree(d["C"])
    run(frozen_vit, d["C"], 2, snapshot_epochs=1)
    half = torch.load(os.path.join(d["C"], ckpt))
    half["rng"]["loader"] = torch.Generator().manual_seed(99).get_state()
    torch.save(half, os.path.join(d["C"], ckpt))
    _, tr_x = run(frozen_vit, d["C"], 4, resume=True)
    assert differs(tr_x.training_state(), state_a)
    # another member index, or a loader of another length, is refused by name
    if kind == "mapping":
        from nested_diffusion_amd.train_mapping import MappingTrainer
        other = MappingTrainer(frozen_vit, 0, num_classes=3, in_features=(IMG // 16) ** 2 * 128, hidden=(48, 32, 16))
        other.run_meta = {k: state_a["meta"][k] for k in ("dataset", "batch_size", "train_batches", "epochs")}
        with pytest.raises(ValueError, match=r"^mn_idx:"):
            other.load_training_state(state_a)
    tr_x.run_meta = dict(tr_x.run_meta, train_batches=5)
    with pytest.raises(ValueError, match=r"^train_batches:"):
        tr_x.load_training_state(state_a)


# ---- 3. the library's sampler state -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_engine_rng_state_restored_repeats_the_next_batch(use_graph):
    from nested_diffusion_amd.engine import EnsembleEngine
    K, D, H, F, C, T, B, mc = 2, 48, 64, 64, 2, 6, 4, 3          # the engine of tests/test_gpu_sampler_refusals.py
    eng = EnsembleEngine(C, D, H, F, 10, n_members=K, max_batch=B, max_rows=B * mc)
    for k in range(K):
        eng.load_member(k, ref_cpu.init_cond_model_params(D, H, F, C, 10, True, seed=70 + k))
    eng.set_schedule(*ref_cpu.schedule_tables("linear", T, 1e-4, 0.02))
    g = torch.Generator().manual_seed(1)
    eng.encode(torch.rand(B, D, generator=g))
    yhat = torch.softmax(torch.randn(K, B, C, generator=g), dim=-1).to(DEV)
    eng.seed(5, first_image=7)
    assert eng.rng_state() == (5, 7 << 32)
    draw = lambda: eng.sample(yhat, yhat, None, mc=mc, T=T, use_graph=use_graph).clone()    # noqa: E731
    first = draw()
    state = eng.rng_state()
    assert state == (5, (7 << 32) | 1)                           # the sampler advanced the batch counter once
    second = draw()
    assert eng.rng_state() == (5, (7 << 32) | 2)
    assert not torch.equal(first, second) and torch.isfinite(second).all()
    third = draw()
    eng.set_rng_state(state)
    assert eng.rng_state() == state
    again = draw()
    assert torch.equal(again, second) and not torch.equal(again, third)
    with pytest.raises(ValueError):
        eng.set_rng_state([1, 2, 3])


# ---- 4. the round trip on the raw images --------------------------------------------------------------------------------------------------
def _bits(t):
    return t.detach().clone().view(torch.int32) if t.dtype == torch.float32 else t.detach().clone()


def _packed_images(trainer_p, m, v):
    from nested_diffusion_amd import ops
    return {f"{w}/{k}": _bits(q.data) for w, src in (("p", trainer_p), ("m", m), ("v", v)) for k, q in src.items()
            if isinstance(q, ops.PackedWeight)}


def test_round_trip_leaves_the_packed_images_bit_identical(frozen_vit):
    """three steps, then load_training_state(training_state()): the raw data of every packed image (parameters and both moments), padding
    rows and lin1's padded columns included; and a trainer built from another seed holds the same images after the load."""
    from nested_diffusion_amd.train_diffusion import NoiseEstimatorTrainer
    from nested_diffusion_amd.train_mapping import MappingTrainer
    from test_gpu_train_mapping import padding_rows
    import _diffusion_train_oracle as oracle_mod
    c = NE
    cfg = config_of(c["B"], c["D"], c["H"], c["F"], c["C"], c["T"])
    tr = NoiseEstimatorTrainer(cfg, DEV, seed=3)
    for s in range(3):
        x, y0, yhat, t, e = oracle_mod.random_batch(c["B"] if s < 2 else 4, c["D"], c["C"], c["T"], seed=20 + s)
        tr.step(x.to(DEV), y0.to(DEV), yhat.to(DEV), t, e.to(DEV))
    before = _packed_images(tr.p, tr.m, tr.v)
    assert len(before) == 3 * 7
    state = tr.training_state()
    tr.load_training_state(state)
    other = NoiseEstimatorTrainer(cfg, DEV, seed=4)
    assert not torch.equal(_bits(other.p["lin2.lin.weight"].data), before["p/lin2.lin.weight"])
    other.load_training_state(state)
    for t2 in (tr, other):
        after = _packed_images(t2.p, t2.m, t2.v)
        assert sorted(after) == sorted(before)
        for k in before:
            assert torch.equal(after[k], before[k]), k
        assert t2.t == 3 and t2.batches_tracked == 3
        pad = padding_rows(t2.p["lin4.weight"])                  # [2, F]: 14 padding rows of 16
        assert pad.numel() == 14 * c["F"] and (pad.contiguous().view(torch.int32) == 0).all()
        assert all(torch.equal(t2.buf[k].cpu(), state["buf"][k]) for k in state["buf"])
    assert same_state(other.training_state(), state) == 3 * 29 + 12
    # the mapping MLP: linear4 [3, 16] has 13 padding rows
    mt = MappingTrainer(frozen_vit, 1, num_classes=3, lr=1e-2, seed=0, in_features=(IMG // 16) ** 2 * 128, hidden=(48, 32, 16))
    x, y, _, _ = image_data(16, 1, 3, IMG, seed=31)
    for lo, hi in ((0, 6), (6, 12), (12, 16)):
        mt.step(x[lo:hi], y[lo:hi])
    before = _packed_images(mt.model.p, mt.m, mt.v)
    assert len(before) == 3 * 4
    state = mt.training_state()
    mt.load_training_state(state)
    other = MappingTrainer(frozen_vit, 1, num_classes=3, lr=1e-2, seed=9, in_features=(IMG // 16) ** 2 * 128, hidden=(48, 32, 16))
    other.load_training_state(state)
    for t2 in (mt, other):
        after = _packed_images(t2.model.p, t2.m, t2.v)
        for k in before:
            assert torch.equal(after[k], before[k]), k
        pad = padding_rows(t2.model.p["linear4.weight"])
        assert pad.numel() == 13 * 16 and (pad.contiguous().view(torch.int32) == 0).all()
        assert t2.t == 3


def test_round_trip_leaves_the_vit_images_bit_identical():
    from nested_diffusion_amd import ops
    from nested_diffusion_amd.train_transformer import ViTTrainer

    def images(tr):
        out = {k: _bits(q.data) for k, q in tr.vit.p.items() if isinstance(q, ops.SplitMatrix)}
        out["pe_w"] = _bits(tr.vit.pe_w.data)
        out.update({"T/" + k: _bits(q.data) for k, q in tr.vit._wT.items()})
        return out

    tr = ViTTrainer(ref_cpu.init_vit_params(embed=128, depth=1, patch=16, img=16, seed=43), num_classes=2, num_heads=2, lr=1e-3)
    x, y, _, _ = image_data(8, 1, 2, 16, seed=32)
    for lo, hi in ((0, 3), (3, 6), (6, 8)):
        tr.step(x[lo:hi], y[lo:hi])
    before = images(tr)
    assert len(before) == 2 * (4 + 1)                            # four block GEMMs and the patch embedding, each with its transpose
    state = tr.training_state()
    tr.load_training_state(state)
    other = ViTTrainer(ref_cpu.init_vit_params(embed=128, depth=1, patch=16, img=16, seed=44), num_classes=2, num_heads=2, lr=1e-3)
    assert not torch.equal(images(other)["pe_w"], before["pe_w"])
    other.load_training_state(state)
    for t2 in (tr, other):
        after = images(t2)
        assert sorted(after) == sorted(before)
        for k in before:
            assert torch.equal(after[k], before[k]), k
        assert t2.t == 3
    assert torch.equal(other.logits(x[:3]), tr.logits(x[:3]))
    assert same_state(other.training_state(), state) == 3 * len(state["p"])
