"""What the trainers share (train_mapping.MappingTrainer, train_transformer.ViTTrainer): StepLR, one pass over a loader for training and
for validation, the reference's epoch loop, and the two command lines' settings, flags and loaders.  The third trainer's loop
(train_diffusion.train_noise_estimator) has its own per-step learning rate and validates by sampling, so it shares no epoch loop; what
it does share lies below both: the snapshot protocol (snapshot.load_run / save_run) and the loader of a split (data.split_loader)."""
from __future__ import annotations

import argparse
import os
import random
from typing import Optional, Tuple

import torch

from . import ops, snapshot
from .data import CACHE_CHOICES, split_loader

VALID_BATCH = 70                      # mapping/data/dataset.py:271: the validation loader's batch
TRAIN_DIR, VALID_DIR = "training", "validation"   # mapping/data/dataset.py:13: data_loader's defaults


def step_lr(lr: float, epoch: int, step_size: int, gamma: float) -> float:
    """StepLR's closed form: the rate during `epoch` (0-based) after `epoch` scheduler steps."""
    return lr * gamma ** (epoch // step_size)


def resolve_settings(args, defaults: dict, max_batch: Optional[int] = None) -> dict:
    """The run's hyper-parameters: the per-dataset defaults with --epochs / --batch_size / --seed applied."""
    s = dict(defaults[args.dataset])
    if args.epochs is not None:
        s["epochs"] = args.epochs
    if args.batch_size is not None:
        s["batch_size"] = args.batch_size
    if s["batch_size"] < 1 or (max_batch is not None and s["batch_size"] > max_batch):
        need = "at least 1" if max_batch is None else f"in [1, {max_batch}]"
        raise SystemExit(f"--batch_size must be {need} (got {s['batch_size']})")
    s["seed"] = random.randint(0, 10000) if args.seed is None else args.seed
    return s


class EpochTrainer:
    """The loop around a trainer's step.  A subclass sets device, base_lr, step_size, gamma and epoch (scheduler steps taken) and supplies
    step(images, labels) -> (loss_sum, n_correct) as device scalars, logits(images), _labels(labels, B) and state_dict(); for snapshots
    also training_state() and load_training_state(state), whose 'meta' carries run_meta (what the loop knows of the run: the dataset,
    the batch size, the training loader's length, the epoch count)."""

    run_meta: dict = {}

    @property
    def lr(self) -> float:
        return step_lr(self.base_lr, self.epoch, self.step_size, self.gamma)

    def scheduler_step(self) -> None:
        self.epoch += 1

    def evaluate(self, loader) -> Tuple[float, float]:
        """(mean loss, accuracy) over a loader, forward only; one read-back at the end."""
        loss_sum = torch.zeros((), dtype=torch.float32, device=self.device)
        correct = torch.zeros((), dtype=torch.int64, device=self.device)
        n = 0
        for images, labels in loader:
            logits = self.logits(images)
            labels = self._labels(labels, logits.shape[0])
            _, loss, _ = ops.ensemble_xent_grad(logits[None], labels, check_labels=False)
            loss_sum += loss.sum()
            correct += (logits.argmax(dim=1) == labels).sum()
            n += logits.shape[0]
        if n == 0:
            raise ValueError("evaluate: the loader is empty")
        return float(loss_sum) / n, int(correct) / n

    def train_epoch(self, loader) -> Tuple[float, float]:
        loss_sum = torch.zeros((), dtype=torch.float32, device=self.device)
        correct = torch.zeros((), dtype=torch.int64, device=self.device)
        n = 0
        for images, labels in loader:
            l, c = self.step(images, labels)
            loss_sum += l
            correct += c
            n += images.shape[0]
        if n == 0:
            raise ValueError("train_epoch: the loader is empty")
        return float(loss_sum) / n, int(correct) / n

    def _fit(self, train_loader, valid_loader, epochs: int, path: str, title: str, snapshot_path: Optional[str] = None,
             snapshot_epochs: int = 0, resume: bool = False) -> dict:
        """mapping/train_mapping.py:92-165, mapping/train_transformer.py:104-172: train epoch, validate, print the two lines, save to
        `path` on a strictly better validation accuracy, then the scheduler step; at the end the line '<title> best train Acc ...'.
        Returns {'best_acc', 'best_train_acc', 'saved_epochs', 'path'}.
        snapshot_path with snapshot_epochs N > 0: after every N-th epoch's scheduler step, and after the last epoch's, the file receives
        {'trainer': training_state(), 'loop': {'next_epoch', 'best_acc', 'best_train_acc', 'saved_epochs'}, 'rng': snapshot.rng_state}
        (snapshot.save_run).  resume: the run starts from that file at the top of epoch 'next_epoch', with every generator where it
        was; the returned dict then covers the earlier epochs too.  The subclass supplies training_state / load_training_state."""
        best_acc, best_train_acc, saved, first = 0.0, 0.0, [], 0
        self.run_meta = dict(self.run_meta, batch_size=snapshot.loader_batch_size(train_loader),
                             train_batches=len(train_loader) if hasattr(train_loader, "__len__") else None, epochs=int(epochs))
        if resume:
            if snapshot_path is None:
                raise ValueError("resume needs a snapshot_path")
            snap = snapshot.load_run(snapshot_path, self)
            loop = snap["loop"]
            first, best_acc, best_train_acc = int(loop["next_epoch"]), float(loop["best_acc"]), float(loop["best_train_acc"])
            saved = [int(e) for e in loop["saved_epochs"]]
            snapshot.set_rng_state(snap["rng"], self.device, train_loader)
            del snap
            print(f"Resumed from {snapshot_path} at epoch {first}")
        for epoch in range(first, int(epochs)):
            tr_loss, tr_acc = self.train_epoch(train_loader)
            print(f"Epoch {epoch} Train Loss: {tr_loss:.4f} Acc: {tr_acc:.4f}")
            va_loss, va_acc = self.evaluate(valid_loader)
            print(f"Epoch {epoch} Test Loss: {va_loss:.4f} Acc: {va_acc:.4f}")
            if va_acc > best_acc:
                best_acc, best_train_acc = va_acc, tr_acc
                os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
                torch.save(self.state_dict(), path)
                saved.append(epoch)
            self.scheduler_step()
            if snapshot_path is not None and snapshot.due(epoch, int(epochs), int(snapshot_epochs)):
                loop = {"next_epoch": epoch + 1, "best_acc": best_acc, "best_train_acc": best_train_acc, "saved_epochs": list(saved)}
                snapshot.save_run(snapshot_path, self, loop, self.device, train_loader)
        print(f"{title} best train Acc: {best_train_acc:.4f} val Acc: {best_acc:.4f}")
        return {"best_acc": best_acc, "best_train_acc": best_train_acc, "saved_epochs": saved, "path": path}


# ---- the two command lines: their shared flags, settings and loaders ------------------------------------------------------------------
def add_cache_flags(ap: argparse.ArgumentParser) -> None:
    """--cache / --cache_dir / --workers: the training input of train_mapping and train_transformer.  A flag that is not given leaves no
    attribute behind (the namespace of a run without them is what it was); cache_settings reads them with their defaults."""
    ap.add_argument("--cache", default=argparse.SUPPRESS, choices=list(CACHE_CHOICES),
                    help="'device': decode every image once, keep both splits on the GPU as bytes and gather each batch there "
                         "(data.DeviceImageSet; same batches, same weights); 'none' (default): a DataLoader decodes every epoch")
    ap.add_argument("--cache_dir", default=argparse.SUPPRESS, help="with --cache device: keep the decoded sets in this directory and reuse them in later runs")
    ap.add_argument("--workers", type=int, default=argparse.SUPPRESS,
                    help="with --cache device: decode threads, at most 16 (default: the CPUs this process may use, at most 16)")


def add_snapshot_flags(ap: argparse.ArgumentParser, where: str) -> None:
    """--snapshot_epochs / --resume of train_mapping and train_transformer; like the cache flags, a flag that is not given leaves no
    attribute behind."""
    ap.add_argument("--snapshot_epochs", type=int, default=argparse.SUPPRESS,
                    help=f"write the whole training state (weights, Adam's moments, counters, generators) to {where} every N epochs and "
                         f"after the last one (default 0: never)")
    ap.add_argument("--resume", action="store_true", default=argparse.SUPPRESS,
                    help=f"continue the run whose state is in {where} (weights, counters and the shuffle's position come from it): same dataset and batch size; --epochs may be larger")


def snapshot_settings(args) -> dict:
    """fit's snapshot_epochs / resume from a parsed command line: 0 and False unless given."""
    n = int(getattr(args, "snapshot_epochs", 0))
    if n < 0:
        raise SystemExit(f"--snapshot_epochs must be at least 0 (got {n})")
    return dict(snapshot_epochs=n, resume=bool(getattr(args, "resume", False)))


def cache_settings(args) -> dict:
    """make_loaders' cache / cache_dir / workers from a parsed command line: 'none', None, None unless given."""
    return dict(cache=getattr(args, "cache", "none"), cache_dir=getattr(args, "cache_dir", None), workers=getattr(args, "workers", None))


def make_loaders(root_dir: str, dataset: str, preprocess: str, batch_size: int, seed: int, cache: str = "none", cache_dir: Optional[str] = None,
                 workers: Optional[int] = None, device=None, image_size=(224, 224)):
    """(training loader, shuffled under the seed; validation loader, batches of VALID_BATCH in file order), each a data.split_loader.
    Unlike the reference's validation loader (drop_last=True) the last partial batch is KEPT: the reference divides by the full dataset
    length either way, so on a set whose size is no multiple of 70 its reported validation accuracy leaves the tail out of the
    numerator; here every image counts.  The accuracy, and with it the epoch whose weights are saved, can therefore differ from the
    reference's on such a set.
    cache='device': the same batches in the same order from data.DeviceImageSet (decoded once by `workers` threads, held on `device`,
    default 'cuda'; images arrive on the device, labels on the CPU); cache_dir keeps the decoded sets as
    <cache_dir>/<split>_<preprocess>_<H>x<W>.npz for later runs."""
    common = dict(cache=cache, cache_dir=cache_dir, device=device, workers=workers)
    g = torch.Generator().manual_seed(int(seed))
    return (split_loader(root_dir, TRAIN_DIR, dataset, preprocess, image_size, batch_size, shuffle=True, generator=g, **common),
            split_loader(root_dir, VALID_DIR, dataset, preprocess, image_size, VALID_BATCH, shuffle=False, **common))
