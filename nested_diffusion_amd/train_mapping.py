"""Training of one mapping MLP on the GPU: mapping/train_mapping.py of the reference, written against this package's operators.

The ViT prefix (patch_embed + blocks[0..mn_idx]) is frozen and runs forward only; the four-layer Classifier on top of it is trained with
cross-entropy (mean over the batch), torch.optim.Adam's update and StepLR.  One step is: the prefix, Classifier.forward_recorded, the
softmax cross-entropy head (nd_ensemble_xent_bwd with one member: a log-softmax), three nd_linear_bwd calls for the hidden gradients, and then -- only
after every gradient that reads a weight has been formed -- one nd_linear_wgrad_adam and one nd_bias_grad_adam per layer, which form the
weight gradient tile by tile and apply Adam to the packed images in place.  No gradient matrix, no unpacked weight and no autograd graph
exists at any point; nothing is read back inside a step.

    python -m nested_diffusion_amd.train_mapping --dataset ChestXRay --root_dir <data> --mn_idx 0 --vit <vit .pth> --out <dir>
writes <dir>/MLPs/block_<mn_idx>.pth (a plain state dict: mapping.load_pickled / load_conditioner read it).  --snapshot_epochs N keeps the
whole training state in <dir>/MLPs/block_<mn_idx>.ckpt (snapshot.py) and --resume continues from it."""
from __future__ import annotations

import argparse
import math
import os
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import _trainer, ops, snapshot
from ._trainer import (TRAIN_DIR, VALID_BATCH, VALID_DIR, EpochTrainer, add_cache_flags, add_snapshot_flags,  # noqa: F401  (this module's interface)
                       cache_settings, make_loaders, snapshot_settings, step_lr)
from .data import cache_file  # noqa: F401  (part of this module's interface)
from .mapping import Classifier, VisionTransformer, load_pickled

MAX_BATCH = ops.LINEAR_BWD_MAX_M      # rows per training step: one nd_linear_bwd / nd_linear_wgrad_adam launch

# mapping/train_mapping.py:46-85 (the two datasets this package has a loader for)
DATASET_DEFAULTS = {
    "ChestXRay": dict(num_classes=2, batch_size=30, lr=1e-3, step_size=20, gamma=0.5, epochs=301),
    "ISICSkinCancer": dict(num_classes=2, batch_size=30, lr=5e-4, step_size=20, gamma=0.5, epochs=100),
}


class MappingTrainer(EpochTrainer):
    """One mapping MLP (mapping/models/mlp.py Classifier: in_features -> hidden[0] -> hidden[1] -> hidden[2] -> num_classes, ReLU between)
    over the frozen prefix of `vit`, with Adam's per-layer m / v images and the step counter beside it."""

    def __init__(self, vit: VisionTransformer, mn_idx: int, num_classes: int = 2, lr: float = 1e-3, step_size: int = 20, gamma: float = 0.5,
                 seed: int = 0, in_features: Optional[int] = None, hidden: Sequence[int] = (4096, 2048, 128)):
        if not 0 <= mn_idx < vit.depth:
            raise ValueError(f"mn_idx must be in [0, {vit.depth}) (mn_idx={mn_idx})")
        if len(hidden) != 3:
            raise ValueError("the Classifier has three hidden layers")
        self.vit, self.mn_idx, self.device = vit, int(mn_idx), vit.device
        self.base_lr, self.step_size, self.gamma = float(lr), int(step_size), float(gamma)
        self.epoch, self.t = 0, 0                           # scheduler steps taken, Adam steps taken
        self.run_meta: Dict[str, object] = {}               # what fit() adds to a snapshot's meta: dataset, batch_size, train_batches, epochs
        if in_features is None:
            in_features = (224 // vit.patch) ** 2 * vit.embed_dim       # vit_base_patch16_224: 196 x 768 = 150528
        dims = [int(in_features), *[int(h) for h in hidden], int(num_classes)]
        gen = torch.Generator(device=self.device)
        gen.manual_seed(int(seed))
        sd: Dict[str, torch.Tensor] = {}
        for i in range(4):                                  # nn.Linear's default: kaiming_uniform(a = sqrt 5) = U(-1/sqrt(fan_in), 1/sqrt(fan_in))
            bound = 1.0 / math.sqrt(dims[i])
            sd[f"linear{i + 1}.weight"] = torch.empty(dims[i + 1], dims[i], dtype=torch.float32, device=self.device).uniform_(-bound, bound, generator=gen)
            sd[f"linear{i + 1}.bias"] = torch.empty(dims[i + 1], dtype=torch.float32, device=self.device).uniform_(-bound, bound, generator=gen)
        self.model = Classifier(sd, self.device)
        self.dims = dims
        del sd
        p = self.model.p
        self.m = {k: (t.zeros_like() if isinstance(t, ops.PackedWeight) else torch.zeros_like(t)) for k, t in p.items()}
        self.v = {k: (t.zeros_like() if isinstance(t, ops.PackedWeight) else torch.zeros_like(t)) for k, t in p.items()}

    def features(self, images: torch.Tensor) -> torch.Tensor:
        """The frozen prefix as compute_guiding_prediction_py runs it: patch_embed, then blocks[0..mn_idx] -> [B, in_features]."""
        images = ops._f32(images.to(self.device), "images")
        B = images.shape[0]
        tok = self.vit.patch_embed(images)
        for i in range(self.mn_idx + 1):
            tok = self.vit.block(i, tok, B)
        return tok.reshape(B, -1)

    def _labels(self, labels: torch.Tensor, B: int) -> torch.Tensor:
        labels = torch.as_tensor(labels).to(device=self.device, dtype=torch.int64)
        if tuple(labels.shape) != (B,):
            raise ValueError(f"labels must be [{B}]")
        return labels

    def step(self, images: torch.Tensor, labels: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """One optimizer step on a batch: (loss_sum, n_correct), both device scalars of the forward BEFORE the update."""
        B = images.shape[0] if images.dim() else 0
        if B < 1:
            raise ValueError("MappingTrainer.step needs a batch of at least one image")
        if B > MAX_BATCH:
            raise ValueError(f"MappingTrainer.step takes batches of at most {MAX_BATCH} rows (B={B}): the weight-gradient kernel sums one "
                             f"batch per launch")
        labels = self._labels(labels, B)
        x = self.features(images)
        if x.shape[1] != self.model.in_features:
            raise ValueError(f"the prefix gives {x.shape[1]} features per image, the Classifier takes {self.model.in_features}")
        p = self.model.p
        logits, acts = self.model.forward_recorded(x)
        _, loss, dlogits = ops.ensemble_xent_grad(logits[None], labels, check_labels=False)
        d4 = dlogits[0]
        d3 = ops.linear_grad_input(d4, p["linear4.weight"], gate=acts[2])
        d2 = ops.linear_grad_input(d3, p["linear3.weight"], gate=acts[1])
        d1 = ops.linear_grad_input(d2, p["linear2.weight"], gate=acts[0])
        # every read of a weight is behind us (same stream): the in-place updates may run
        a = ops.adam_step(self.lr, self.t + 1)
        gscale = 1.0 / B                                    # nn.CrossEntropyLoss's mean
        for i, (dy, inp) in enumerate(((d1, x), (d2, acts[0]), (d3, acts[1]), (d4, acts[2])), start=1):
            kw, kb = f"linear{i}.weight", f"linear{i}.bias"
            ops.linear_wgrad_adam(dy, inp, p[kw], self.m[kw], self.v[kw], a, gscale=gscale)
            ops.bias_grad_adam(dy, p[kb], self.m[kb], self.v[kb], a, gscale=gscale)
        self.t += 1                                         # counted once all eight updates are enqueued
        return loss.sum(), (logits.argmax(dim=1) == labels).sum()

    def logits(self, images: torch.Tensor) -> torch.Tensor:
        return self.model(self.features(images))

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """The reference's keys linear{1..4}.{weight,bias}, weights unpacked to [N, K], on the CPU."""
        return {k: (t.unpack() if isinstance(t, ops.PackedWeight) else t).detach().cpu().clone() for k, t in self.model.p.items()}

    # ---- the whole training state, for snapshots (snapshot.py) ---------------------------------------------------------------------
    def _meta(self) -> dict:
        return dict({"format": snapshot.FORMAT, "kind": "mapping", "mn_idx": self.mn_idx, "in_features": self.dims[0], "hidden": self.dims[1:4],
                     "num_classes": self.dims[4]}, **self.run_meta)

    def training_state(self) -> dict:
        """{'meta', 'p', 'm', 'v' (Adam's moments under the parameters' keys), 't', 'epoch'}: on the CPU, row-major, the reference's keys
        and shapes.  One image is unpacked, copied out and released at a time."""
        out = lambda q: (q.unpack() if isinstance(q, ops.PackedWeight) else q).detach().cpu()    # noqa: E731
        state = {"meta": self._meta()}
        for which, src in (("p", self.model.p), ("m", self.m), ("v", self.v)):
            state[which] = {k: out(src[k]) for k in Classifier.KEYS}
        state.update(t=int(self.t), epoch=int(self.epoch))
        return state

    def load_training_state(self, state: dict) -> None:
        """training_state() of a run with this run's meta (snapshot.check_meta: a ValueError names the field that differs), put back bit
        for bit; the packed images are rebuilt from the row-major tensors, one at a time, after every shape has been checked."""
        snapshot.check_meta(state.get("meta"), self._meta())
        for which in ("p", "m", "v"):
            for i in range(4):
                for k, shape in ((f"linear{i + 1}.weight", (self.dims[i + 1], self.dims[i])), (f"linear{i + 1}.bias", (self.dims[i + 1],))):
                    if k not in state[which] or tuple(state[which][k].shape) != shape:
                        raise ValueError(f"{which}['{k}'] is missing or has another shape than {shape}")
        for which, dst in (("p", self.model.p), ("m", self.m), ("v", self.v)):
            for k in Classifier.KEYS:
                w = state[which][k].detach().to(self.device, torch.float32).contiguous()
                if isinstance(dst[k], ops.PackedWeight):
                    dst[k] = None                            # the old image goes before the new one is built
                    dst[k] = ops.PackedWeight(w)
                else:
                    dst[k].copy_(w)
                del w
        self.t, self.epoch = int(state["t"]), int(state["epoch"])

    def fit(self, train_loader, valid_loader, epochs: int, out_dir: str, snapshot_path: Optional[str] = None, snapshot_epochs: int = 0,
            resume: bool = False, dataset: Optional[str] = None) -> dict:
        """mapping/train_mapping.py:92-165 (EpochTrainer._fit), saving <out_dir>/MLPs/block_<mn_idx>.pth.  snapshot_epochs N: the whole
        training state goes to snapshot_path (default <out_dir>/MLPs/block_<mn_idx>.ckpt) every N epochs and after the last; resume: the
        run continues from that file."""
        path = os.path.join(out_dir, "MLPs", f"block_{self.mn_idx}.pth")
        if snapshot_path is None and (snapshot_epochs or resume):
            snapshot_path = path[:-4] + ".ckpt"
        self.run_meta = dict(self.run_meta, dataset=dataset)
        return self._fit(train_loader, valid_loader, epochs, path, f"MLP {self.mn_idx}", snapshot_path=snapshot_path,
                         snapshot_epochs=snapshot_epochs, resume=resume)


def build_parser() -> argparse.ArgumentParser:
    """The reference's flag names, types and choices (the two datasets this package has a loader for), plus --vit, --out, --epochs and
    --batch_size, and the training input's --cache, --cache_dir and --workers."""
    ap = argparse.ArgumentParser(prog="python -m nested_diffusion_amd.train_mapping",
                                 description="Train one mapping MLP over a frozen ViT prefix on the GPU (fused HIP weight gradient + Adam).")
    ap.add_argument("--seed", type=int, default=None, help="seed of the weight draw and of the training loader's shuffle (default: drawn at random)")
    ap.add_argument("--dataset", required=True, choices=sorted(DATASET_DEFAULTS), help="selects the hyper-parameters and the normalisation constants")
    ap.add_argument("--root_dir", required=True, help=f"image tree holding {TRAIN_DIR}/<class>/ and {VALID_DIR}/<class>/")
    ap.add_argument("--preprocess", default="grayscaled", choices=["grayscaled", "standardized"], help="input transform of data.ImageFolderDataset")
    ap.add_argument("--mn_idx", type=int, required=True, choices=[0, 1, 2, 3, 4], help="k: the MLP reads the tokens after ViT block k")
    ap.add_argument("--vit", required=True, help="ViT checkpoint: a state dict or a whole-module pickle (mapping.load_pickled)")
    ap.add_argument("--out", required=True, help="directory that receives MLPs/block_<mn_idx>.pth")
    ap.add_argument("--epochs", type=int, default=None, help="default: per dataset (DATASET_DEFAULTS)")
    ap.add_argument("--batch_size", type=int, default=None, help=f"training batch, at most {MAX_BATCH}; default: per dataset (DATASET_DEFAULTS)")
    add_cache_flags(ap)
    add_snapshot_flags(ap, "<out>/MLPs/block_<mn_idx>.ckpt")
    return ap


def resolve_settings(args) -> dict:
    """The run's hyper-parameters: the per-dataset defaults with --epochs / --batch_size (at most MAX_BATCH) / --seed applied."""
    return _trainer.resolve_settings(args, DATASET_DEFAULTS, MAX_BATCH)


def main(argv=None) -> dict:
    args = build_parser().parse_args(argv)
    s = resolve_settings(args)
    if not torch.cuda.is_available():
        raise SystemExit("train_mapping needs a GPU (no CPU fallback)")
    print(f"Training Mapping Network {args.mn_idx} on {args.root_dir}")
    vit_sd = load_pickled(args.vit)
    vit = VisionTransformer(vit_sd, max(1, vit_sd["patch_embed.proj.weight"].shape[0] // 64), "cuda")
    train_loader, valid_loader = make_loaders(args.root_dir, args.dataset, args.preprocess, s["batch_size"], s["seed"], **cache_settings(args))
    trainer = MappingTrainer(vit, args.mn_idx, num_classes=s["num_classes"], lr=s["lr"], step_size=s["step_size"], gamma=s["gamma"],
                             seed=s["seed"])
    return trainer.fit(train_loader, valid_loader, s["epochs"], args.out, dataset=args.dataset, **snapshot_settings(args))


if __name__ == "__main__":
    main()
