"""Host-side checks of the resumable training runs (nested_diffusion_amd/snapshot.py and its callers; no GPU): the meta check names the
field that differs and lets the epoch count grow, the atomic write keeps the previous file when the write fails, the three command lines
without the new flags parse to the namespaces they had, `main --resume_training` without a snapshot names the file it looked for, and
EpochTrainer._fit with its default arguments writes no snapshot."""
import argparse
import os

import pytest
import torch

from test_trainer_loop_host import make_stub

META = {"format": 1, "kind": "noise_estimator", "num_classes": 2, "data_dim": 48, "hidden_dim": 32, "feature_dim": 32, "timesteps": 6,
        "mlp_idx": 1, "dataset": "ChestXRay", "batch_size": 6, "train_batches": 3, "epochs": 4}


# ---- 1. the meta check --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field,other", [("kind", "mapping"), ("num_classes", 3), ("data_dim", 64), ("hidden_dim", 48), ("feature_dim", 16),
                                         ("timesteps", 7), ("mlp_idx", 2), ("dataset", "ISICSkinCancer"), ("batch_size", 8),
                                         ("train_batches", 4), ("format", 2)])
def test_check_meta_refuses_each_mismatching_field_by_name(field, other):
    from nested_diffusion_amd.snapshot import check_meta
    check_meta(dict(META), dict(META))
    with pytest.raises(ValueError, match=rf"^{field}:"):
        check_meta(dict(META, **{field: other}), dict(META))


def test_check_meta_accepts_a_larger_epoch_count_and_refuses_a_missing_field():
    from nested_diffusion_amd.snapshot import check_meta
    check_meta(dict(META), dict(META, epochs=400))
    check_meta(dict(META, epochs=400), dict(META))
    saved = dict(META)
    del saved["mlp_idx"]
    with pytest.raises(ValueError, match=r"^mlp_idx:"):
        check_meta(saved, dict(META))
    with pytest.raises(ValueError, match=r"^meta:"):
        check_meta(None, dict(META))
    for kind, key in (("mapping", "mn_idx"), ("vit", "embed_dim")):                 # the other trainers' fields go through the same loop
        mine = {"format": 1, "kind": kind, key: 2}
        with pytest.raises(ValueError, match=rf"^{key}:"):
            check_meta(dict(mine, **{key: 3}), mine)


# ---- 2. the atomic write ------------------------------------------------------------------------------------------------------------------
def test_atomic_save_keeps_the_old_file_when_the_write_fails(tmp_path, monkeypatch):
    from nested_diffusion_amd import snapshot
    path = str(tmp_path / "sub" / "ckpt.pth")
    snapshot.atomic_save({"v": torch.arange(3)}, path)                             # makes the directory
    assert os.listdir(os.path.dirname(path)) == ["ckpt.pth"]
    save = torch.save

    def failing_save(obj, f, *a, **kw):
        save({"half": 1}, f)                                                       # something reaches the disk, then the write dies
        raise OSError("disk full")

    monkeypatch.setattr(torch, "save", failing_save)
    with pytest.raises(OSError, match="disk full"):
        snapshot.atomic_save({"v": torch.arange(4)}, path)
    monkeypatch.setattr(torch, "save", save)
    assert os.listdir(os.path.dirname(path)) == ["ckpt.pth"]                       # no .tmp left behind
    assert torch.equal(torch.load(path)["v"], torch.arange(3))
    snapshot.atomic_save({"v": torch.arange(5)}, path)
    assert torch.equal(torch.load(path)["v"], torch.arange(5)) and os.listdir(os.path.dirname(path)) == ["ckpt.pth"]


def test_read_names_a_missing_file_and_refuses_a_file_that_is_no_snapshot(tmp_path):
    from nested_diffusion_amd import snapshot
    missing = str(tmp_path / "nothing.ckpt")
    with pytest.raises(FileNotFoundError) as e:
        snapshot.read(missing)
    assert missing in str(e.value)
    other = str(tmp_path / "weights.pth")
    torch.save({"linear1.weight": torch.zeros(2, 2)}, other)
    with pytest.raises(ValueError, match="not a training snapshot"):
        snapshot.read(other)


def test_due_every_n_epochs_and_after_the_last():
    from nested_diffusion_amd.snapshot import due
    assert [e for e in range(7) if due(e, 7, 3)] == [2, 5, 6]
    assert [e for e in range(4) if due(e, 4, 1)] == [0, 1, 2, 3]
    assert not any(due(e, 4, 0) for e in range(4))


def test_loader_generator_finds_the_generator_or_none():
    from nested_diffusion_amd.data import IndexBatchLoader, SyntheticLoader
    from nested_diffusion_amd.snapshot import loader_batch_size, loader_generator
    g = torch.Generator().manual_seed(3)
    data = list(range(10))
    assert loader_generator(torch.utils.data.DataLoader(data, batch_size=4, shuffle=True, generator=g)) is g
    assert loader_generator(torch.utils.data.DataLoader(data, batch_size=4, shuffle=True)) is None
    assert loader_generator(IndexBatchLoader(data, 4, shuffle=True, generator=g)) is g
    assert loader_generator(IndexBatchLoader(data, 4, shuffle=True)) is None
    assert loader_generator([(0, 1)]) is None and loader_generator(SyntheticLoader(2, 4, 2)) is None
    assert loader_batch_size(IndexBatchLoader(data, 4)) == 4 and loader_batch_size(SyntheticLoader(2, 6, 2)) == 6
    assert loader_batch_size([(0, 1)]) is None


def test_abi_carries_the_sampler_state_pair_and_refuses_null_before_any_hip_call():
    import ctypes
    from nested_diffusion_amd import _lib
    for name in ("nd_rng_state", "nd_set_rng_state"):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 2, name
    lib = _lib.load()
    st = (ctypes.c_uint64 * 2)(1, 2)
    h = ctypes.c_void_p()
    assert lib.nd_create(ctypes.byref(_lib.NdConfig(2, 48, 64, 64, 10, 1, 4, 4)), ctypes.byref(h)) == 0
    try:
        for fn in (lib.nd_rng_state, lib.nd_set_rng_state):
            assert fn(None, st) == -1 and b"NULL" in lib.nd_last_error()
            assert fn(h, None) == -1 and b"NULL" in lib.nd_last_error()
            assert fn(h, st) == -3 and b"workspace not bound" in lib.nd_last_error()      # created, nothing bound: no device is touched
        assert (st[0], st[1]) == (1, 2)
    finally:
        lib.nd_destroy(h)


# ---- 3. the command lines -----------------------------------------------------------------------------------------------------------------
MAIN_KEYS = ['add_ce_loss', 'attack_name', 'brightness', 'cache_dir', 'calib', 'comment', 'config', 'contrast', 'covered', 'crop', 'dataroot',
             'device', 'doc', 'eps', 'eta', 'eval_best', 'exp', 'fid', 'fp16', 'image_folder', 'interpolation', 'loss', 'low_mem_mode',
             'low_resolution', 'mc_trials', 'mlp_idx', 'n_splits', 'ni', 'no_cat_f_phi', 'noise_perturbation', 'noise_prior', 'num_sample',
             'preprocess', 'resume_training', 'sample', 'sample_type', 'sanity_check', 'seed', 'sequence', 'skip_type', 'split',
             'synthetic_batches', 'test', 'test_sample_seed', 'thread', 'timesteps', 'train_cache', 'train_guidance_only', 'tune_T', 'verbose']


def test_parsers_without_the_new_flags_give_the_namespaces_they_gave_before():
    from nested_diffusion_amd import main as nd_main, train_mapping as tm, train_transformer as tt
    ns = tm.build_parser().parse_args("--dataset ChestXRay --root_dir r --mn_idx 0 --vit v --out o".split())
    assert vars(ns) == {'seed': None, 'dataset': 'ChestXRay', 'root_dir': 'r', 'preprocess': 'grayscaled', 'mn_idx': 0, 'vit': 'v', 'out': 'o',
                        'epochs': None, 'batch_size': None}
    assert tm.snapshot_settings(ns) == {"snapshot_epochs": 0, "resume": False}
    ns = tt.build_parser().parse_args("--dataset ChestXRay --root_dir r --out o".split())
    assert vars(ns) == {'seed': None, 'dataset': 'ChestXRay', 'root_dir': 'r', 'preprocess': 'grayscaled', 'out': 'o', 'init': None,
                        'epochs': None, 'batch_size': None}
    ns = nd_main.build_parser().parse_args("--config c --doc d --preprocess grayscaled".split())
    assert sorted(vars(ns)) == MAIN_KEYS and ns.resume_training is False
    # and with them
    ns = tm.build_parser().parse_args("--dataset ChestXRay --root_dir r --mn_idx 0 --vit v --out o --snapshot_epochs 5 --resume".split())
    assert tm.snapshot_settings(ns) == {"snapshot_epochs": 5, "resume": True}
    ns = tt.build_parser().parse_args("--dataset ChestXRay --root_dir r --out o --snapshot_epochs 2".split())
    assert tm.snapshot_settings(ns) == {"snapshot_epochs": 2, "resume": False}
    ns = nd_main.build_parser().parse_args("--config c --doc d --preprocess grayscaled --snapshot_epochs 10 --resume_training".split())
    assert ns.snapshot_epochs == 10 and ns.resume_training is True
    with pytest.raises(SystemExit):
        tm.snapshot_settings(argparse.Namespace(snapshot_epochs=-1))


def test_resume_training_without_a_snapshot_names_the_missing_path(tmp_path):
    """Diffusion.train reads the snapshot before it builds anything: a runner that holds no device state gets as far as the refusal."""
    from nested_diffusion_amd.runner import Diffusion
    ns = argparse.Namespace
    runner = object.__new__(Diffusion)
    runner.args = ns(log_path=str(tmp_path), resume_training=True, snapshot_epochs=1)
    runner.config = ns(diffusion=ns(aux_cls=ns(arch="sevit")))
    runner.cond_pred_model = ns(mlps=[None, None])
    runner.operand_dtype = "f32"
    with pytest.raises(FileNotFoundError) as e:
        runner.train(0, train_loader=[], valid_loader=[])
    assert os.path.join(str(tmp_path), "ckpt.pth") in str(e.value)


# ---- 4. the loop's defaults ---------------------------------------------------------------------------------------------------------------
def test_fit_with_default_arguments_writes_no_snapshot(tmp_path, capsys):
    tr = make_stub([0.5, 0.75])
    res = tr._fit("TRAIN", "VALID", 2, str(tmp_path / "best.pth"), "Stub")
    assert res["saved_epochs"] == [0, 1] and sorted(os.listdir(str(tmp_path))) == ["best.pth"]
    # a path alone (snapshot_epochs 0) writes none either
    tr = make_stub([0.5, 0.75])
    tr._fit(["T"], "VALID", 2, str(tmp_path / "best.pth"), "Stub", snapshot_path=str(tmp_path / "best.ckpt"))
    assert sorted(os.listdir(str(tmp_path))) == ["best.pth"]
    capsys.readouterr()


# ---- 5. the run protocol: snapshot.load_run / save_run, and the loop that calls them ---------------------------------------------------------
@pytest.fixture
def rng_recorders(monkeypatch):
    """snapshot.rng_state / set_rng_state touch the GPU generator: recorders in their place"""
    from nested_diffusion_amd import snapshot
    calls = []
    monkeypatch.setattr(snapshot, "rng_state", lambda device, loader, engine=None: (calls.append(("get", device, loader, engine)), {"tag": 7})[1])
    monkeypatch.setattr(snapshot, "set_rng_state", lambda state, device, loader, engine=None: calls.append(("set", state, device, loader, engine)))
    return calls


class StateStub:
    def __init__(self):
        self.loaded = []

    def training_state(self):
        return {"meta": {"format": 1}, "p": {"w": torch.arange(4.0)}, "t": 3}

    def load_training_state(self, state):
        self.loaded.append(state)


def test_load_run_and_save_run_round_trip_on_a_stub_trainer(tmp_path, rng_recorders):
    from nested_diffusion_amd import snapshot
    path, tr = str(tmp_path / "run" / "ckpt.pth"), StateStub()
    snapshot.save_run(path, tr, {"next_epoch": 2, "step": 6}, "dev", "LOADER", "ENGINE")
    assert rng_recorders == [("get", "dev", "LOADER", "ENGINE")]
    assert sorted(torch.load(path)) == ["loop", "rng", "trainer"] and os.listdir(os.path.dirname(path)) == ["ckpt.pth"]
    snap = snapshot.load_run(path, tr)
    assert sorted(snap) == ["loop", "rng", "trainer"] and snap["loop"] == {"next_epoch": 2, "step": 6} and snap["rng"] == {"tag": 7}
    assert len(tr.loaded) == 1 and tr.loaded[0] is snap["trainer"]
    got, want = tr.loaded[0], tr.training_state()
    assert sorted(got) == sorted(want) and got["meta"] == want["meta"] and got["t"] == 3 and torch.equal(got["p"]["w"], want["p"]["w"])
    assert len(rng_recorders) == 1                                                 # load_run leaves the generators to its caller
    # a missing file is refused before the trainer is touched; a file without 'loop' is read's ValueError
    fresh, missing = StateStub(), str(tmp_path / "run" / "none.pth")
    with pytest.raises(FileNotFoundError) as e:
        snapshot.load_run(missing, fresh)
    assert missing in str(e.value) and fresh.loaded == []
    torch.save({"trainer": want, "rng": {"tag": 7}}, missing)
    with pytest.raises(ValueError, match="not a training snapshot: it has no 'loop' entry"):
        snapshot.load_run(missing, fresh)
    assert fresh.loaded == []


def test_fit_resumed_from_the_epoch_2_snapshot_ends_as_the_straight_run(tmp_path, capsys, rng_recorders):
    import shutil
    accs, ckpt, aside = [0.5, 0.5, 0.75, 0.6], str(tmp_path / "best.ckpt"), str(tmp_path / "after_epoch_1.ckpt")

    def stub(copy_at=None):
        tr = make_stub(accs)
        tr.training_state = lambda: {"epoch": tr.epoch}
        tr.load_training_state = lambda state: setattr(tr, "epoch", int(state["epoch"]))
        evaluate = tr.evaluate

        def evaluate_and_copy(loader):
            if tr.epoch == copy_at:                                                # the third epoch: the file holds the state after the second
                shutil.copy(ckpt, aside)
            return evaluate(loader)

        tr.evaluate = evaluate_and_copy
        return tr

    straight = stub(copy_at=2)._fit("TRAIN", "VALID", 4, str(tmp_path / "best.pth"), "Stub", snapshot_path=ckpt, snapshot_epochs=2)
    lines_a = capsys.readouterr().out.splitlines()
    assert [c[0] for c in rng_recorders] == ["get", "get"] and all(c[1:] == ("cpu", "TRAIN", None) for c in rng_recorders)
    half = torch.load(aside)
    assert sorted(half) == ["loop", "rng", "trainer"] and sorted(half["loop"]) == ["best_acc", "best_train_acc", "next_epoch", "saved_epochs"]
    assert half["loop"]["next_epoch"] == 2 and half["trainer"] == {"epoch": 2} and torch.load(ckpt)["loop"]["next_epoch"] == 4
    del rng_recorders[:]
    tr = stub()
    resumed = tr._fit("TRAIN", "VALID", 4, str(tmp_path / "best.pth"), "Stub", snapshot_path=aside, snapshot_epochs=2, resume=True)
    lines_b = capsys.readouterr().out.splitlines()
    assert resumed == straight and resumed["saved_epochs"] == [0, 2]
    assert rng_recorders[0] == ("set", {"tag": 7}, "cpu", "TRAIN", None) and [c[0] for c in rng_recorders[1:]] == ["get"]
    assert tr.calls == [("train", "TRAIN"), ("valid", "VALID")] * 2                # epochs 2 and 3 only
    assert lines_b[0] == f"Resumed from {aside} at epoch 2"
    assert lines_b[1:] == lines_a[4:] and len(lines_a) == 9 and lines_b[1].startswith("Epoch 2 Train") and lines_b[3].startswith("Epoch 3 Train")
