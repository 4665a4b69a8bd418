"""Training of the ViT on the GPU: mapping/train_transformer.py of the reference (model_type 'vit'), written against this package's operators.

Every parameter of timm's vit_base_patch16_224 is trained with cross-entropy (mean over the batch), torch.optim.AdamW's update over one
parameter group and StepLR.  One step is: VisionTransformer._forward_recorded (the forward of forward(): every dropout and drop-path rate
of the model is 0, so model.train() computes what eval computes), the softmax cross-entropy head, the input-gradient chain of the attacks
with its fp32 gradients kept (nd_layernorm_bwd, nd_gelu_bwd_split, nd_attention_bwd, nd_gemm_split on the transposed weight images), and
per parameter ONE fused launch -- nd_gemm_tn_adamw for a Linear weight, nd_colsum_adamw for a bias, pos_embed and cls_token,
nd_layernorm_wgrad_adamw for a LayerNorm -- which forms the gradient and applies AdamW in place.  The GEMM weights live twice: as row-major
fp32 masters (what AdamW updates) and as the frag32b3 images the forward and the backward read; the images are rewritten in place from the
masters once the last gradient of the step has been formed.  No gradient matrix and no autograd graph exists at any point; nothing is read
back inside a step.

    python -m nested_diffusion_amd.train_transformer --dataset ChestXRay --root_dir <data> --out <dir>
writes <dir>/vit_base_patch16_224_<Dataset>.pth (a plain timm-keyed state dict: mapping.load_pickled / load_conditioner and
train_mapping --vit read it).  --snapshot_epochs N keeps the whole training state in <dir>/vit_base_patch16_224_<Dataset>.ckpt (snapshot.py)
and --resume continues from it."""
from __future__ import annotations

import argparse
import math
import os
from typing import Dict, Optional, Tuple

import torch

from . import _trainer, ops, snapshot
from ._trainer import (TRAIN_DIR, VALID_DIR, EpochTrainer, add_cache_flags, add_snapshot_flags, cache_settings, make_loaders, snapshot_settings,
                       step_lr)  # noqa: F401  (step_lr, make_loaders: part of this module's interface)
from .mapping import LN_EPS, VisionTransformer, load_pickled, require_fp32_split

# mapping/train_transformer.py:47-49, 95-97 (the two datasets this package has a loader for)
DATASET_DEFAULTS = {
    "ChestXRay": dict(num_classes=2, batch_size=30, lr=1e-4, weight_decay=0.1, step_size=10, gamma=0.5, epochs=200),
    "ISICSkinCancer": dict(num_classes=2, batch_size=30, lr=1e-4, weight_decay=0.1, step_size=10, gamma=0.5, epochs=200),
}
SAVE_MODEL_NAME = "vit_base_patch16_224"                  # mapping/train_transformer.py:78


def checkpoint_path(out_dir: str, dataset: str) -> str:
    """<out>/vit_base_patch16_224_<Dataset>.pth: the file mapping.load_conditioner and attack.make_attacks read."""
    return os.path.join(out_dir, f"{SAVE_MODEL_NAME}_{dataset}.pth")


def _trunc_normal(shape, std: float, gen: torch.Generator) -> torch.Tensor:
    """N(0, std^2) cut at two standard deviations, by the inverse CDF (torch.nn.init.trunc_normal_'s method), drawn in double."""
    lo, hi = math.erf(-2.0 / math.sqrt(2.0)), math.erf(2.0 / math.sqrt(2.0))          # 2 Phi(-2) - 1, 2 Phi(2) - 1
    t = torch.empty(shape, dtype=torch.float64).uniform_(lo, hi, generator=gen)
    return t.erfinv_().mul_(std * math.sqrt(2.0)).clamp_(-2.0 * std, 2.0 * std).to(torch.float32)


def _uniform(shape, bound: float, gen: torch.Generator) -> torch.Tensor:
    return torch.empty(shape, dtype=torch.float32).uniform_(-bound, bound, generator=gen)


def init_state_dict(num_classes: int = 2, embed: int = 768, depth: int = 12, patch: int = 16, img: int = 224, in_chans: int = 3,
                    mlp_ratio: int = 4, seed: int = 0) -> Dict[str, torch.Tensor]:
    """A fresh timm-keyed state dict (CPU, fp32), restating timm 0.4.12 create_model('vit_base_patch16_224', pretrained=False) followed by
    the reference's fresh head (mapping/train_transformer.py:76-77): block Linear weights, pos_embed and cls_token trunc_normal(std 0.02,
    cut at two standard deviations), Linear biases 0, LayerNorm 1 / 0, the patch-embedding conv and the replaced head torch's nn.Conv2d /
    nn.Linear default U(-1/sqrt(fan_in), 1/sqrt(fan_in)) for weight and bias.  timm is not installed here: parity unpinned (the
    distributions are restated from its source, the draws are this function's own)."""
    gen = torch.Generator().manual_seed(int(seed))
    n_tok = (img // patch) ** 2 + 1
    sd: Dict[str, torch.Tensor] = {}
    sd["cls_token"] = _trunc_normal((1, 1, embed), 0.02, gen)
    sd["pos_embed"] = _trunc_normal((1, n_tok, embed), 0.02, gen)
    fan = in_chans * patch * patch
    sd["patch_embed.proj.weight"] = _uniform((embed, in_chans, patch, patch), 1.0 / math.sqrt(fan), gen)
    sd["patch_embed.proj.bias"] = _uniform((embed,), 1.0 / math.sqrt(fan), gen)
    widths = {"attn.qkv": (3 * embed, embed), "attn.proj": (embed, embed), "mlp.fc1": (mlp_ratio * embed, embed),
              "mlp.fc2": (embed, mlp_ratio * embed)}
    for i in range(depth):
        pre = f"blocks.{i}."
        for name in ("norm1", "attn.qkv", "attn.proj", "norm2", "mlp.fc1", "mlp.fc2"):
            if name.startswith("norm"):
                sd[pre + name + ".weight"] = torch.ones(embed)
                sd[pre + name + ".bias"] = torch.zeros(embed)
            else:
                sd[pre + name + ".weight"] = _trunc_normal(widths[name], 0.02, gen)
                sd[pre + name + ".bias"] = torch.zeros(widths[name][0])
    sd["norm.weight"] = torch.ones(embed)
    sd["norm.bias"] = torch.zeros(embed)
    sd.update(_fresh_head(num_classes, embed, gen))
    return sd


def _fresh_head(num_classes: int, embed: int, gen: torch.Generator) -> Dict[str, torch.Tensor]:
    bound = 1.0 / math.sqrt(embed)
    return {"head.weight": _uniform((num_classes, embed), bound, gen), "head.bias": _uniform((num_classes,), bound, gen)}


class ViTTrainer(EpochTrainer):
    """timm's VisionTransformer with AdamW's m / v for every parameter and the step counter beside it.  state_dict None: a fresh model
    (init_state_dict; **arch are its widths).  A state dict whose head has another class count gets the reference's fresh head."""

    def __init__(self, state_dict: Optional[Dict[str, torch.Tensor]], num_classes: int = 2, num_heads: int = 12, lr: float = 1e-4,
                 weight_decay: float = 0.1, step_size: int = 10, gamma: float = 0.5, seed: int = 0, device="cuda", dtype="f32", **arch):
        require_fp32_split("ViTTrainer", dtype=dtype)                   # before anything is built
        if state_dict is None:
            sd = init_state_dict(num_classes, seed=seed, **arch)
        else:
            if arch:
                raise ValueError(f"{sorted(arch)} describe a fresh model; a state dict brings its own widths")
            sd = {k: v for k, v in state_dict.items() if torch.is_tensor(v) and v.is_floating_point()}
            if sd["head.weight"].shape[0] != num_classes:
                sd.update(_fresh_head(num_classes, sd["head.weight"].shape[1], torch.Generator().manual_seed(int(seed))))
        self.vit = VisionTransformer(sd, num_heads, device)
        require_fp32_split("ViTTrainer", vit=self.vit)
        self.device = self.vit.device
        self.base_lr, self.weight_decay, self.step_size, self.gamma = float(lr), float(weight_decay), int(step_size), float(gamma)
        self.epoch, self.t = 0, 0                               # scheduler steps taken, AdamW steps taken
        self.run_meta: Dict[str, object] = {}                   # what fit() adds to a snapshot's meta: dataset, batch_size, train_batches, epochs
        p = self.vit.p
        # the row-major fp32 masters of the weights the ViT holds as images only; every other parameter is its own master in vit.p
        self.master = {k: sd[k].detach().to(self.device, torch.float32).contiguous().clone() for k, t in p.items()
                       if isinstance(t, ops.SplitMatrix)}
        self.m = {k: torch.zeros_like(self._param(k)) for k in p}
        self.v = {k: torch.zeros_like(self._param(k)) for k in p}
        self.vit.transposed_weights()

    def _param(self, k: str) -> torch.Tensor:
        """The fp32 tensor AdamW updates for state-dict key k."""
        return self.master[k] if k in self.master else self.vit.p[k]

    def _labels(self, labels: torch.Tensor, B: int, check_range: bool = False) -> torch.Tensor:
        labels = torch.as_tensor(labels)
        if tuple(labels.shape) != (B,):
            raise ValueError(f"labels must be [{B}]")
        C = self.vit.p["head.weight"].shape[0]
        if B and (check_range or not labels.is_cuda) and (int(labels.min()) < 0 or int(labels.max()) >= C):   # no read-back for a CPU tensor
            raise ValueError(f"labels must lie in [0, {C})")
        return labels.to(device=self.device, dtype=torch.int64).contiguous()

    # ---- one pass: forward, backward chain, and per parameter one gradient / fused launch ---------------------------------------------
    def _pass(self, images: torch.Tensor, labels: torch.Tensor, a, check_range: bool):
        """a: an ops.adamw_step (fused: every parameter is updated, returns no gradients) or None (gradient-only: returns them)."""
        images = ops._f32(torch.as_tensor(images).to(self.device), "images")
        if images.dim() != 4 or images.shape[0] < 1:
            raise ValueError("images must be [B >= 1, C, H, W]")
        vit, p, grads = self.vit, self.vit.p, {}
        labels = self._labels(labels, images.shape[0], check_range)
        logits, cls_in, recs, B, N, H, W = vit._forward_recorded(images)
        E, gscale, fused = vit.embed_dim, 1.0 / images.shape[0], a is not None

        def gemm(k, dy, x):
            w = self._param(k)
            g = ops.gemm_tn_adamw(dy, x, w.view(w.shape[0], -1) if fused else None, self.m[k].view(w.shape[0], -1) if fused else None,
                                  self.v[k].view(w.shape[0], -1) if fused else None, a, gscale=gscale, return_grad=not fused)
            if not fused:
                grads[k] = g.reshape(w.shape)

        def colsum(k, dy):
            g = ops.colsum_adamw(dy, p[k] if fused else None, self.m[k] if fused else None, self.v[k] if fused else None, a, gscale=gscale,
                                 return_grad=not fused)
            if not fused:
                grads[k] = g.reshape(p[k].shape)

        def norm(pre, x, g):
            kw, kb = pre + ".weight", pre + ".bias"
            r = ops.layernorm_wgrad_adamw(x, g, LN_EPS, p[kw] if fused else None, p[kb] if fused else None, self.m[kw] if fused else None,
                                          self.v[kw] if fused else None, self.m[kb] if fused else None, self.v[kb] if fused else None, a,
                                          gscale=gscale, return_grad=not fused)
            if not fused:
                grads[kw], grads[kb] = r

        # the head: dlogits for its own parameters, dcls (= dlogits . head.weight, input_grad's kernel) for everything below
        _, loss, dlogits = ops.ensemble_xent_grad(logits[None], labels, check_labels=False)
        dlogits = dlogits[0]
        dcls, _ = ops.xent_head_grad(logits, labels, p["head.weight"], check_labels=False)
        cls = ops.layernorm(cls_in, p["norm.weight"], p["norm.bias"], LN_EPS)

        def stage(i, r, dy, g):
            """The parameter launches of one stage of the chain, issued right after its chain launches (a parameter is updated only after
            everything that reads it in this step has been enqueued: same stream).  dy: dL/d(the stage's output)."""
            if r is None:                                     # the top: the head and the final norm
                gemm("head.weight", dlogits, cls)
                colsum("head.bias", dlogits)
                norm("norm", cls_in, dy)
                return
            pre = f"blocks.{i}."
            # the Linear inputs the forward did not keep in fp32
            gelu, _ = ops.gelu_split(r["u"], want_out=True)
            h2 = ops.layernorm(r["x2"], p[pre + "norm2.weight"], p[pre + "norm2.bias"], LN_EPS)
            h1 = ops.layernorm(r["x"], p[pre + "norm1.weight"], p[pre + "norm1.bias"], LN_EPS)
            gemm(pre + "mlp.fc2.weight", dy, gelu)
            colsum(pre + "mlp.fc2.bias", dy)
            gemm(pre + "mlp.fc1.weight", g["du"], h2)
            colsum(pre + "mlp.fc1.bias", g["du"])
            norm(pre + "norm2", r["x2"], g["dh2"])
            gemm(pre + "attn.proj.weight", g["dx2"], r["o"])
            colsum(pre + "attn.proj.bias", g["dx2"])
            gemm(pre + "attn.qkv.weight", g["dqkv"], h1)
            colsum(pre + "attn.qkv.bias", g["dqkv"])
            norm(pre + "norm1", r["x"], g["dh1"])

        dy = vit._token_backward(dcls, cls_in, recs, B, N, per_block=stage)
        tokg = dy.reshape(B, N, E)
        colsum("pos_embed", dy.reshape(B, N * E))
        colsum("cls_token", tokg[:, 0].contiguous())
        dpatch = tokg[:, 1:].reshape(-1, E).contiguous()
        gemm("patch_embed.proj.weight", dpatch, ops.patchify(images, vit.patch))
        colsum("patch_embed.proj.bias", dpatch)
        if fused:
            self._refresh_images()
        return grads, loss, logits, labels

    def _refresh_images(self) -> None:
        """The frag32b3 images of the updated GEMM weights and of their transposes, rewritten in place (their addresses stay: an nd_cond
        handle bound to them sees the new weights)."""
        vit = self.vit
        pe = vit.p["patch_embed.proj.weight"]                  # its own master (vit.p keeps the 4-D fp32 tensor; the image is vit.pe_w)
        for k, w2, img in [(k, w, vit.p[k]) for k, w in self.master.items()] + [("patch_embed", pe.view(pe.shape[0], -1), vit.pe_w)]:
            ops.split_rows(w2, out=img)
            if getattr(vit, "_wT", None) is not None:
                ops.split_rows(w2.t().contiguous(), out=vit._wT[k])

    def gradients(self, images: torch.Tensor, labels: torch.Tensor):
        """(grads, loss [B], logits): the gradient of the MEAN cross-entropy at every parameter, keyed by the timm state-dict names in
        their shapes; nothing is updated.  The logits equal vit.forward(images) bit for bit."""
        grads, loss, logits, _ = self._pass(images, labels, None, True)
        return grads, loss, logits

    def step(self, images: torch.Tensor, labels: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """One optimizer step on a batch: (loss_sum, n_correct), both device scalars of the forward BEFORE the update."""
        a = ops.adamw_step(self.lr, self.t + 1, self.weight_decay)
        _, loss, logits, labels = self._pass(images, labels, a, False)
        self.t += 1                                         # counted once every update is enqueued
        return loss.sum(), (logits.argmax(dim=1) == labels).sum()

    def logits(self, images: torch.Tensor) -> torch.Tensor:
        return self.vit.forward(ops._f32(torch.as_tensor(images).to(self.device), "images"))

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """timm's keys in timm's shapes (the patch-embedding weight 4-D), on the CPU."""
        return {k: self._param(k).detach().cpu().clone() for k in self.vit.p}

    # ---- the whole training state, for snapshots (snapshot.py) ---------------------------------------------------------------------
    def _meta(self) -> dict:
        vit, p = self.vit, self.vit.p
        return dict({"format": snapshot.FORMAT, "kind": "vit", "embed_dim": vit.embed_dim, "depth": vit.depth, "patch": vit.patch,
                     "in_chans": vit.in_chans, "tokens": p["pos_embed"].shape[1], "num_classes": p["head.weight"].shape[0]}, **self.run_meta)

    def training_state(self) -> dict:
        """{'meta', 'p' (the fp32 masters, timm's keys and shapes), 'm', 'v' (AdamW's moments under the same keys), 't', 'epoch'} on the
        CPU, one tensor copied out at a time.  The frag32b3 images are not in it: they are a function of the masters."""
        state = {"meta": self._meta(), "p": {k: self._param(k).detach().cpu() for k in self.vit.p}}
        for which, src in (("m", self.m), ("v", self.v)):
            state[which] = {k: src[k].detach().cpu() for k in self.vit.p}
        state.update(t=int(self.t), epoch=int(self.epoch))
        return state

    def load_training_state(self, state: dict) -> None:
        """training_state() of a run with this run's meta (snapshot.check_meta: a ValueError names the field that differs), copied into
        the masters and moments in place after every shape has been checked; the frag32b3 images and their transposes are then rewritten
        from the masters as at the end of a step (_refresh_images)."""
        snapshot.check_meta(state.get("meta"), self._meta())
        for which in ("p", "m", "v"):
            for k in self.vit.p:
                if k not in state[which] or tuple(state[which][k].shape) != tuple(self._param(k).shape):
                    raise ValueError(f"{which}['{k}'] is missing or has another shape than {tuple(self._param(k).shape)}")
        for k in self.vit.p:
            self._param(k).copy_(state["p"][k])
            self.m[k].copy_(state["m"][k])
            self.v[k].copy_(state["v"][k])
        self._refresh_images()
        self.t, self.epoch = int(state["t"]), int(state["epoch"])

    def fit(self, train_loader, valid_loader, epochs: int, out_dir: str, dataset: str, snapshot_path: Optional[str] = None,
            snapshot_epochs: int = 0, resume: bool = False) -> dict:
        """mapping/train_transformer.py:104-172 (EpochTrainer._fit), saving checkpoint_path(out_dir, dataset).  snapshot_epochs N: the
        whole training state goes to snapshot_path (default: that path with the extension .ckpt) every N epochs and after the last;
        resume: the run continues from that file."""
        path = checkpoint_path(out_dir, dataset)
        if snapshot_path is None and (snapshot_epochs or resume):
            snapshot_path = path[:-4] + ".ckpt"
        self.run_meta = dict(self.run_meta, dataset=dataset)
        return self._fit(train_loader, valid_loader, epochs, path, f"Model vit on {dataset}", snapshot_path=snapshot_path,
                         snapshot_epochs=snapshot_epochs, resume=resume)


def build_parser() -> argparse.ArgumentParser:
    """The reference's flag names, types and choices (the two datasets this package has a loader for; model_type is always 'vit'), plus
    --out, --init, --epochs and --batch_size, and the training input's --cache, --cache_dir and --workers."""
    ap = argparse.ArgumentParser(prog="python -m nested_diffusion_amd.train_transformer",
                                 description="Train the ViT on the GPU (HIP backward chain, fused weight gradient + AdamW).")
    ap.add_argument("--seed", type=int, default=None, help="seed of the weight draw and of the training loader's shuffle (default: drawn at random)")
    ap.add_argument("--dataset", required=True, choices=sorted(DATASET_DEFAULTS), help="selects the class count, the batch and the normalisation constants")
    ap.add_argument("--root_dir", required=True, help=f"image tree holding {TRAIN_DIR}/<class>/ and {VALID_DIR}/<class>/")
    ap.add_argument("--preprocess", default="grayscaled", choices=["grayscaled", "standardized"], help="input transform of data.ImageFolderDataset")
    ap.add_argument("--out", required=True, help=f"directory that receives {SAVE_MODEL_NAME}_<Dataset>.pth")
    ap.add_argument("--init", default=None, help="start from this ViT checkpoint (a state dict or a whole-module pickle) instead of a fresh model")
    ap.add_argument("--epochs", type=int, default=None, help="default: per dataset (DATASET_DEFAULTS)")
    ap.add_argument("--batch_size", type=int, default=None, help="training batch; default: per dataset (DATASET_DEFAULTS)")
    add_cache_flags(ap)
    add_snapshot_flags(ap, f"<out>/{SAVE_MODEL_NAME}_<Dataset>.ckpt")
    return ap


def resolve_settings(args) -> dict:
    """The run's hyper-parameters: the per-dataset defaults with --epochs / --batch_size / --seed applied."""
    return _trainer.resolve_settings(args, DATASET_DEFAULTS)


def main(argv=None) -> dict:
    args = build_parser().parse_args(argv)
    s = resolve_settings(args)
    if not torch.cuda.is_available():
        raise SystemExit("train_transformer needs a GPU (no CPU fallback)")
    print(f"Training vit on {args.root_dir} with seed {s['seed']}:")
    sd = load_pickled(args.init) if args.init else None
    heads = max(1, sd["patch_embed.proj.weight"].shape[0] // 64) if sd is not None else 12
    trainer = ViTTrainer(sd, num_classes=s["num_classes"], num_heads=heads, lr=s["lr"], weight_decay=s["weight_decay"],
                         step_size=s["step_size"], gamma=s["gamma"], seed=s["seed"])
    train_loader, valid_loader = make_loaders(args.root_dir, args.dataset, args.preprocess, s["batch_size"], s["seed"], **cache_settings(args))
    return trainer.fit(train_loader, valid_loader, s["epochs"], args.out, args.dataset, **snapshot_settings(args))


if __name__ == "__main__":
    main()
