"""The epoch loop the two trainers share (nested_diffusion_amd/_trainer.py EpochTrainer), on a stub with scripted epochs: no GPU."""
import os

import pytest
import torch


def make_stub(va_accs):
    from nested_diffusion_amd._trainer import EpochTrainer

    class Stub(EpochTrainer):
        def __init__(self):
            self.device, self.base_lr, self.step_size, self.gamma, self.epoch = "cpu", 1e-3, 2, 0.5, 0
            self.calls, self.lrs, self.saved_at = [], [], []

        def train_epoch(self, loader):
            self.calls.append(("train", loader))
            self.lrs.append(self.lr)
            return 1.0 / (self.epoch + 1), 0.1 * (self.epoch + 1)          # (loss, accuracy): epoch e trains to accuracy 0.1 (e + 1)

        def evaluate(self, loader):
            self.calls.append(("valid", loader))
            return 2.0, va_accs[self.epoch]

        def state_dict(self):
            self.saved_at.append(self.epoch)
            return {"epoch": torch.tensor(self.epoch)}

    return Stub()


def test_fit_saves_on_strictly_better_accuracy_and_prints_in_order(tmp_path, capsys):
    tr = make_stub([0.5, 0.5, 0.75, 0.6])
    path = str(tmp_path / "not" / "yet" / "there.pth")
    res = tr._fit("TRAIN", "VALID", 4, path, "Stub 7")
    assert res["saved_epochs"] == [0, 2] and tr.saved_at == [0, 2]            # an equal accuracy (epoch 1) and a worse one (3) save nothing
    assert res["best_acc"] == 0.75 and res["best_train_acc"] == pytest.approx(0.3) and res["best_train_acc"] == 0.1 * 3
    assert res["path"] == path and sorted(res) == ["best_acc", "best_train_acc", "path", "saved_epochs"]
    assert tr.epoch == 4                                                      # the scheduler was stepped once per epoch
    assert tr.lrs == [1e-3, 1e-3, 5e-4, 5e-4]                                 # ... after the epoch's training, StepLR(2, 0.5)
    assert tr.calls == [("train", "TRAIN"), ("valid", "VALID")] * 4
    assert os.path.isdir(os.path.dirname(path)) and int(torch.load(path)["epoch"]) == 2
    assert capsys.readouterr().out.splitlines() == [
        "Epoch 0 Train Loss: 1.0000 Acc: 0.1000", "Epoch 0 Test Loss: 2.0000 Acc: 0.5000",
        "Epoch 1 Train Loss: 0.5000 Acc: 0.2000", "Epoch 1 Test Loss: 2.0000 Acc: 0.5000",
        "Epoch 2 Train Loss: 0.3333 Acc: 0.3000", "Epoch 2 Test Loss: 2.0000 Acc: 0.7500",
        "Epoch 3 Train Loss: 0.2500 Acc: 0.4000", "Epoch 3 Test Loss: 2.0000 Acc: 0.6000",
        "Stub 7 best train Acc: 0.3000 val Acc: 0.7500"]


def test_the_trainers_fit_is_the_shared_loop(tmp_path, capsys):
    """MappingTrainer.fit(..., out_dir) and ViTTrainer.fit(..., out_dir, dataset) only name the checkpoint and the last line"""
    from nested_diffusion_amd import train_mapping as tm, train_transformer as tt
    from nested_diffusion_amd._trainer import EpochTrainer
    assert issubclass(tm.MappingTrainer, EpochTrainer) and issubclass(tt.ViTTrainer, EpochTrainer)
    for cls in (tm.MappingTrainer, tt.ViTTrainer):
        for name in ("lr", "scheduler_step", "evaluate", "train_epoch", "_fit"):
            assert name not in vars(cls), (cls, name)
    stub = make_stub([0.5])
    stub.mn_idx = 3
    res = tm.MappingTrainer.fit(stub, "T", "V", 1, str(tmp_path / "a"))
    assert res["path"] == os.path.join(str(tmp_path / "a"), "MLPs", "block_3.pth") and os.path.exists(res["path"])
    assert capsys.readouterr().out.splitlines()[-1] == "MLP 3 best train Acc: 0.1000 val Acc: 0.5000"
    stub = make_stub([0.5])
    res = tt.ViTTrainer.fit(stub, "T", "V", 1, str(tmp_path / "b"), "ChestXRay")
    assert res["path"] == tt.checkpoint_path(str(tmp_path / "b"), "ChestXRay") and os.path.exists(res["path"])
    assert capsys.readouterr().out.splitlines()[-1] == "Model vit on ChestXRay best train Acc: 0.1000 val Acc: 0.5000"


def test_an_empty_loader_is_refused_by_the_real_passes():
    from nested_diffusion_amd._trainer import EpochTrainer

    class Bare(EpochTrainer):
        device = "cpu"

    for name in ("evaluate", "train_epoch"):
        with pytest.raises(ValueError, match=f"{name}: the loader is empty"):
            getattr(Bare(), name)([])
        with pytest.raises(ValueError, match="empty"):
            getattr(Bare(), name)(iter(()))
