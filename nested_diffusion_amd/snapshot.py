"""Full-state snapshots of a training run, so that an interrupted run continues instead of starting over.  One file:

    {'trainer': trainer.training_state(), 'loop': {...the epoch loop's counters...}, 'rng': {...every generator the loop draws from...}}

written at epoch boundaries only (after the epoch's validation, its best-checkpoint save and its scheduler step), so a resumed run starts
at the top of an epoch.  Everything in the file is on the CPU, row-major, in the reference's keys and shapes: it does not depend on how
the device holds the weights.  Host code throughout: the pure functions here (check_meta, atomic_save, read, loader_generator) need
neither a GPU nor the library."""
from __future__ import annotations

import os
from typing import Dict, Optional

import torch

FORMAT = 1
KINDS = ("noise_estimator", "mapping", "vit")
EXTENDABLE = ("epochs",)          # recorded for the reader, never compared: a resumed run may ask for more epochs than the first one did
OPTIONAL = ("ema_rate",)          # recorded only by a run that has it (an EMA shadow): a snapshot with one belongs to no run without


def check_meta(saved: dict, expected: dict) -> None:
    """Does a snapshot's 'meta' belong to this run?  Raises a ValueError that names the first field that differs: the format, the kind
    of trainer, a dimension, the member index (mlp_idx / mn_idx), the dataset, the batch size or the training loader's length
    (train_batches), the EMA rate (ema_rate: recorded by a run that keeps a shadow, and then refused by one that keeps none as well as
    the reverse).  The epoch count is not compared: a run can be extended."""
    if not isinstance(saved, dict):
        raise ValueError("meta: the snapshot holds no 'meta' entry")
    if saved.get("format") != FORMAT:
        raise ValueError(f"format: the snapshot has format {saved.get('format')!r}, this build reads format {FORMAT}")
    for field, want in expected.items():
        if field in EXTENDABLE or field == "format":
            continue
        if field not in saved:
            raise ValueError(f"{field}: the snapshot does not record it (this run has {field}={want!r})")
        if saved[field] != want:
            raise ValueError(f"{field}: the snapshot was taken with {field}={saved[field]!r}, this run has {field}={want!r}")
    for field in OPTIONAL:
        if field in saved and field not in expected:
            raise ValueError(f"{field}: the snapshot was taken with {field}={saved[field]!r}, this run has none")


def atomic_save(obj, path: str) -> None:
    """torch.save to <path>.tmp, then os.replace: a write that fails, or a process that dies inside it, leaves the previous snapshot as
    it was."""
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    tmp = path + ".tmp"
    try:
        torch.save(obj, tmp)
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.unlink(tmp)
        raise


def require(path: str) -> None:
    """A FileNotFoundError that names the path when there is no snapshot at `path`: what a loop asks before it builds anything."""
    if not os.path.isfile(path):
        raise FileNotFoundError(f"cannot resume: there is no snapshot at {path}")


def read(path: str) -> dict:
    """The snapshot at `path`, on the CPU; require()'s FileNotFoundError when there is none."""
    require(path)
    snap = torch.load(path, map_location="cpu", weights_only=True)
    for part in ("trainer", "loop", "rng"):
        if not isinstance(snap, dict) or part not in snap:
            raise ValueError(f"{path} is not a training snapshot: it has no '{part}' entry")
    return snap


def due(epoch: int, n_epochs: int, snapshot_epochs: int) -> bool:
    """Is a snapshot written after `epoch` (0-based)?  Every snapshot_epochs epochs and after the last one; never with snapshot_epochs 0."""
    return snapshot_epochs > 0 and ((epoch + 1) % snapshot_epochs == 0 or epoch + 1 == n_epochs)


def loader_generator(loader) -> Optional[torch.Generator]:
    """The generator a training loader shuffles with: DataLoader.generator, or that of the index loader inside a data.IndexBatchLoader;
    None when it has none (it then draws from the global CPU generator) or is no loader of those kinds (a list of batches)."""
    inner = getattr(loader, "indices", None)
    if isinstance(inner, torch.utils.data.DataLoader):
        loader = inner
    gen = getattr(loader, "generator", None)
    return gen if isinstance(gen, torch.Generator) else None


def loader_batch_size(loader) -> Optional[int]:
    """The batch size of a DataLoader / data.IndexBatchLoader / data.SyntheticLoader, None where the loader does not say."""
    inner = getattr(loader, "indices", None)
    if isinstance(inner, torch.utils.data.DataLoader):
        loader = inner
    b = getattr(loader, "batch_size", None)
    if b is None:
        b = getattr(loader, "global_batch", None)
    return int(b) if isinstance(b, int) else None


def rng_state(device, train_loader, engine=None) -> Dict[str, object]:
    """Everything the loops draw from: the global CPU generator (antithetic_timesteps; a DataLoader without a generator), the trainer
    device's generator (e = randn), the training loader's own generator if it has one, and the in-library sampler state of the
    validation engine if there is one (two 64-bit words, kept as Python ints)."""
    gen = loader_generator(train_loader)
    return {"cpu": torch.get_rng_state(), "cuda": torch.cuda.get_rng_state(device),
            "loader": gen.get_state() if gen is not None else None,
            "engine": list(engine.rng_state()) if engine is not None else None}


def set_rng_state(state: dict, device, train_loader, engine=None) -> None:
    """Put rng_state()'s streams back.  A snapshot that holds a loader generator's state needs a loader that has one, and the reverse."""
    gen = loader_generator(train_loader)
    if (gen is None) != (state.get("loader") is None):
        raise ValueError("loader generator: the snapshot " + ("holds" if gen is None else "does not hold") + " the state of a training "
                         "loader's own generator, this run's loader " + ("has none" if gen is None else "has one"))
    torch.set_rng_state(state["cpu"])
    torch.cuda.set_rng_state(state["cuda"], device)
    if gen is not None:
        gen.set_state(state["loader"])
    if engine is not None and state.get("engine") is not None:
        engine.set_rng_state(state["engine"])


# ---- the run protocol of the epoch loops (_trainer.EpochTrainer._fit, train_diffusion.train_noise_estimator) -----------------------------
def load_run(path: str, trainer) -> dict:
    """Resume, first half: read(path) -- so a missing file is refused before the trainer is touched -- and
    trainer.load_training_state(snap['trainer']).  Returns the snapshot: the loop takes its counters from snap['loop'] and, once it has
    its training loader (and its validation engine, if it samples), calls set_rng_state(snap['rng'], ...)."""
    snap = read(path)
    trainer.load_training_state(snap["trainer"])
    return snap


def save_run(path: str, trainer, loop: dict, device, train_loader, engine=None) -> None:
    """The file of the module docstring, written at the end of an epoch: the trainer's whole state, the loop's counters for the top of
    the next epoch, and rng_state(device, train_loader, engine)."""
    atomic_save({"trainer": trainer.training_state(), "loop": loop, "rng": rng_state(device, train_loader, engine)}, path)
