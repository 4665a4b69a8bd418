"""Training of one noise estimator on the GPU: Diffusion.train of diffusion/classification_train_separately.py:842-1141 for
latent_model.py's ConditionalModel (arch 'linear', guidance=True), written against this package's operators.

Host side, as pure functions (no GPU, no library): lr_at (the learning-rate schedule), antithetic_timesteps (the timestep draw),
cast_label_to_one_hot_and_prototype (the label encoding) and check_step_args (every refusal of a step, BEFORE anything is launched).

Device side, NoiseEstimatorTrainer: one step is the seven Linear layers on the packed weight images (ops.linear), each BatchNorm1d in
training mode fused with ConditionalLinear's per-timestep gain, the softplus and the product with xe (ops.bn_train_forward), q_sample
with host-gathered coefficients and the mean-squared error (ops.qsample, ops.mse_grad), then back through ops.bn_train_backward and
ops.linear_grad_input.  clip_grad_norm_ needs the norm of ALL gradients before the first parameter moves, so Adam cannot be fused into
the weight-gradient pass as it is for the mapping MLPs: the 29 gradients are materialised (the gradient-only mode of
ops.linear_wgrad_adam / ops.bias_grad_adam for the Linear layers), their squares summed in a fixed order (ops.sumsq), and ops.clip_adam
scales and applies them.  All of it is fp32 arithmetic in documented orders, except that the BatchNorm kernels carry a column's statistics
and sums in double (include/nested_diffusion.h says why).  Nothing is read back inside a step; no torch gather or index op runs on the device: the timesteps stay on the
CPU until check_step_args has passed them, and the schedule coefficients of a batch are gathered there.

The EMA shadow (diffusion/ema.py; registered at :879-883, updated after every optimizer step at :1006-1011) is kept on request:
NoiseEstimatorTrainer(..., ema_rate=mu) clones every parameter at construction, each ops.clip_adam call of a step then carries the
parameter's shadow through the same pass (nd_clip_adam_ema: no second read of the weights), ema_state_dict() is what the reference's
EMA.ema(model); model.state_dict() gives, and training_state() / load_training_state() carry the shadow as 'ema'.  It costs one more
copy of the parameters on the device.  Without a rate nothing of it exists: the same launches, allocations and state keys as ever.
The reference never reads its shadow back in training -- the checkpoint saves noise_estimator.state_dict() (:1120) -- so the shadow
changes nothing else a run writes.  Out of scope: train_guidance_only, more than one GPU, the fp16 mode.  training_state() /
load_training_state() carry a run across an interruption (snapshot.py; train_noise_estimator writes and reads the file).

The loop around the step, train_noise_estimator (what runner.Diffusion.train runs): train_request refuses, validate samples the validation
set with the current weights, save_best writes the inference checkpoint."""
from __future__ import annotations

import logging
import math
import os
from typing import Dict, Optional, Tuple

import torch

from . import dist as nd_dist, ops, snapshot
from .data import split_loader
from .diffusion_utils import schedule_tables
from .engine import EnsembleEngine
from .latent_model import LIN1_K, check_member_dims, member_shapes, pad_lin1


def lr_at(epoch: float, config) -> float:
    """adjust_learning_rate of diffusion/utils.py:83-96 as a pure function: a linear warm-up over training.warmup_epochs, then a
    half-cycle cosine from optim.lr down to optim.min_lr at training.n_epochs.  `epoch` is fractional: i / len(loader) + epoch."""
    warm, total = config.training.warmup_epochs, config.training.n_epochs
    if epoch < warm:
        return config.optim.lr * epoch / warm
    return config.optim.min_lr + (config.optim.lr - config.optim.min_lr) * 0.5 * (1.0 + math.cos(math.pi * (epoch - warm) / (total - warm)))


def antithetic_timesteps(n: int, num_timesteps: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """:945-948: n // 2 + 1 draws t from [0, T), joined with T - 1 - t and cut to n (int64, on the CPU: the draw is host plumbing and its
    range is known without a read-back)."""
    t = torch.randint(low=0, high=num_timesteps, size=(n // 2 + 1,), generator=generator)
    return torch.cat([t, num_timesteps - 1 - t], dim=0)[:n]


def cast_label_to_one_hot_and_prototype(y_labels_batch, config, return_prototype: bool = True):
    """diffusion/utils.py:244-255: the one-hot float labels [B, C] and, if asked for, their logit prototypes (the one-hot clipped to
    data.label_min_max, L1-normalised per row, through logit).  The training loop uses the one-hot alone."""
    y_one_hot = torch.nn.functional.one_hot(torch.as_tensor(y_labels_batch).long(), num_classes=config.data.num_classes).float()
    if not return_prototype:
        return y_one_hot, None
    lo, hi = config.data.label_min_max
    return y_one_hot, torch.logit(torch.nn.functional.normalize(torch.clip(y_one_hot, min=lo, max=hi), p=1.0, dim=1))


MIN_BATCH, MAX_BATCH = 2, 128         # BatchNorm's batch statistics need two rows; one nd_linear_bwd / nd_linear_wgrad_adam launch takes 128

BN_NAMES = ("encoder_x.1", "encoder_x.4", "norm", "unetnorm1", "unetnorm2", "unetnorm3")
# ConditionalModel.parameters() in registration order (latent_model.py:127-167): the order clip_grad_norm_ and Adam walk, and the order
# in which the squares of the gradients are summed
PARAM_KEYS = ("encoder_x.0.weight", "encoder_x.0.bias", "encoder_x.1.weight", "encoder_x.1.bias", "encoder_x.3.weight", "encoder_x.3.bias",
              "encoder_x.4.weight", "encoder_x.4.bias", "encoder_x.6.weight", "encoder_x.6.bias", "norm.weight", "norm.bias",
              "lin1.lin.weight", "lin1.lin.bias", "lin1.embed.weight", "unetnorm1.weight", "unetnorm1.bias",
              "lin2.lin.weight", "lin2.lin.bias", "lin2.embed.weight", "unetnorm2.weight", "unetnorm2.bias",
              "lin3.lin.weight", "lin3.lin.bias", "lin3.embed.weight", "unetnorm3.weight", "unetnorm3.bias", "lin4.weight", "lin4.bias")
PACKED_KEYS = ("encoder_x.0.weight", "encoder_x.3.weight", "encoder_x.6.weight", "lin1.lin.weight", "lin2.lin.weight", "lin3.lin.weight",
               "lin4.weight")


def check_step_args(x_flat, y0, yhat, t, e, data_dim: int, num_classes: int, num_timesteps: int) -> int:
    """Every refusal of a training step, as a pure function of its arguments (nothing is launched, nothing is uploaded): the batch size
    B.  x_flat [B, data_dim], y0 / yhat / e [B, num_classes] float32; t [B] an int64 tensor ON THE CPU with every entry in
    [0, num_timesteps); 2 <= B <= 128.  Raises ValueError otherwise."""
    for a, name in ((x_flat, "x_flat"), (y0, "y0"), (yhat, "yhat"), (e, "e"), (t, "t")):
        if not torch.is_tensor(a):
            raise ValueError(f"{name} must be a tensor")
    if t.device.type != "cpu" or t.dtype != torch.int64 or t.dim() != 1:
        raise ValueError(f"t must be a one-dimensional int64 tensor on the CPU (it is uploaded as int32 only after its range has been "
                         f"checked); got {t.dtype} {tuple(t.shape)} on {t.device}")
    B = t.shape[0]
    if not MIN_BATCH <= B <= MAX_BATCH:
        raise ValueError(f"a training step takes {MIN_BATCH} <= B <= {MAX_BATCH} rows (B={B}): BatchNorm's batch statistics need two, the "
                         f"weight-gradient kernel sums one batch per launch")
    if x_flat.dtype != torch.float32 or tuple(x_flat.shape) != (B, data_dim):
        raise ValueError(f"x_flat must be float32 [{B}, {data_dim}]; got {x_flat.dtype} {tuple(x_flat.shape)}")
    for a, name in ((y0, "y0"), (yhat, "yhat"), (e, "e")):
        if a.dtype != torch.float32 or tuple(a.shape) != (B, num_classes):
            raise ValueError(f"{name} must be float32 [{B}, {num_classes}]; got {a.dtype} {tuple(a.shape)}")
    lo, hi = int(t.min()), int(t.max())
    if lo < 0 or hi >= num_timesteps:
        raise ValueError(f"every timestep must lie in [0, {num_timesteps}); got [{lo}, {hi}]")
    return B


def _refuse_config(config) -> None:
    """Only what the shipped configs use is built; everything else refuses by name."""
    if config.model.arch != "linear":
        raise NotImplementedError(f"model.arch == {config.model.arch!r}: only 'linear' is implemented")
    if not getattr(config.diffusion, "include_guidance", True):
        raise NotImplementedError("diffusion.include_guidance == False: only ConditionalModel(guidance=True) is implemented")
    optim = getattr(config, "optim", None)
    if optim is not None:
        if getattr(optim, "optimizer", "Adam") != "Adam":
            raise NotImplementedError(f"optim.optimizer == {optim.optimizer!r}: only 'Adam' is implemented")
        if getattr(optim, "weight_decay", 0.0) or getattr(optim, "amsgrad", False):
            raise NotImplementedError("optim.weight_decay != 0 / optim.amsgrad: only plain Adam is implemented")


class NoiseEstimatorTrainer:
    """One ConditionalModel(config, guidance=True) in training mode with Adam's state beside it.  The seven Linear weights live as packed
    images (ops.PackedWeight); lin1.lin.weight [F, 2C] is held padded to LIN1_K columns and its input cat(y_t, yhat) zero-padded to match:
    the padded columns' gradient is exactly +0 and Adam leaves them at 0; state_dict() cuts them off.  `lr` is the learning rate of the
    next step (the loop sets it from lr_at); every other hyper-parameter comes from config.optim.  ema_rate: keep the EMA shadow of every
    parameter at that rate in self.shadow (None: no shadow, and nothing of it in any launch, allocation or saved state)."""

    def __init__(self, config, device, seed: int = 0, state_dict: Optional[Dict[str, torch.Tensor]] = None,
                 ema_rate: Optional[float] = None):
        _refuse_config(config)
        self.ema_rate = None if ema_rate is None else float(ema_rate)
        if self.ema_rate is not None:
            ops.ema_step(self.ema_rate)                                             # refuses a rate outside (0, 1) before anything is built
        self.device = torch.device(device)
        self.C, self.D = int(config.data.num_classes), int(config.model.data_dim)
        self.H, self.F, self.T = int(config.model.hidden_dim), int(config.model.feature_dim), int(config.diffusion.timesteps)
        C, D, H, F, T = self.C, self.D, self.H, self.F, self.T
        check_member_dims(C, D, H, F, T)
        optim = getattr(config, "optim", None)
        self.lr = float(getattr(optim, "lr", 1e-3))
        self.betas = (float(getattr(optim, "beta1", 0.9)), 0.999)                   # diffusion/utils.py:55
        self.eps = float(getattr(optim, "eps", 1e-8))
        clip = getattr(optim, "grad_clip", 1.0)
        self.grad_clip = float(clip)
        self.t = 0                                                                  # Adam steps taken = num_batches_tracked
        self.run_meta: Dict[str, object] = {}      # what the loop adds to a snapshot's meta: mlp_idx, dataset, batch_size, train_batches, epochs
        # the schedule tables q_sample reads (classification_train_separately.py:215-226), on the CPU: a batch's rows are gathered there
        tables = schedule_tables(getattr(config.diffusion, "beta_schedule", "linear"), T, getattr(config.diffusion, "beta_start", 1e-4),
                                 getattr(config.diffusion, "beta_end", 0.02))
        self.alphas_bar_sqrt, self.one_minus_alphas_bar_sqrt = tables.alphas_bar_sqrt, tables.one_minus_alphas_bar_sqrt
        shapes = self.shapes()
        sd = self._initial_state(seed) if state_dict is None else state_dict
        dev = self.device
        self.p: Dict[str, object] = {}
        self.buf: Dict[str, torch.Tensor] = {}
        for k in PARAM_KEYS:
            if k not in sd:
                raise KeyError(f"state_dict is missing '{k}'")
            w = sd[k].detach().to(dev, torch.float32).contiguous()
            if tuple(w.shape) != shapes[k]:
                raise ValueError(f"'{k}' has shape {tuple(w.shape)}, expected {shapes[k]}")
            if k == "lin1.lin.weight":
                w = pad_lin1(w)
            self.p[k] = ops.PackedWeight(w) if k in PACKED_KEYS else w.clone()
        for name in BN_NAMES:
            n = shapes[name + ".weight"][0]
            for stat, fill in (("running_mean", 0.0), ("running_var", 1.0)):
                key = f"{name}.{stat}"
                if state_dict is not None and key in state_dict:
                    b = state_dict[key].detach().to(dev, torch.float32).contiguous().clone()
                    if tuple(b.shape) != (n,):
                        raise ValueError(f"'{key}' has shape {tuple(b.shape)}, expected ({n},)")
                else:
                    b = torch.full((n,), fill, dtype=torch.float32, device=dev)
                self.buf[key] = b
        if state_dict is not None and "norm.num_batches_tracked" in state_dict:
            self.batches_tracked = int(state_dict["norm.num_batches_tracked"])
        else:
            self.batches_tracked = 0
        zeros = lambda q: q.zeros_like() if isinstance(q, ops.PackedWeight) else torch.zeros_like(q)    # noqa: E731
        self.m = {k: zeros(q) for k, q in self.p.items()}
        self.v = {k: zeros(q) for k, q in self.p.items()}
        # EMA.register right after the model is built (:880-881): a clone of every parameter, packed images staying packed
        self.shadow: Optional[Dict[str, object]] = None
        if self.ema_rate is not None:
            self.shadow = {k: self._clone(q) for k, q in self.p.items()}
        self.last_sumsq: Optional[torch.Tensor] = None       # the device scalar the last step clipped with (sum of all squared gradients)

    @staticmethod
    def _clone(q):
        """a second buffer with q's bits: a tensor, or a packed image copied as it lies (padding rows included)"""
        if not isinstance(q, ops.PackedWeight):
            return q.clone()
        c = object.__new__(ops.PackedWeight)
        c.N, c.K, c.dtype, c.data = q.N, q.K, q.dtype, q.data.clone()
        return c

    def shapes(self) -> Dict[str, Tuple[int, ...]]:
        return member_shapes(self.C, self.D, self.H, self.F, self.T)

    def _initial_state(self, seed: int) -> Dict[str, torch.Tensor]:
        """nn.Linear's default U(-1/sqrt(fan_in), 1/sqrt(fan_in)) for weight and bias, Embedding.uniform_(0, 1) (latent_model.py:99),
        BatchNorm gamma = 1, beta = 0, drawn on the device under `seed` in PARAM_KEYS order."""
        gen = torch.Generator(device=self.device)
        gen.manual_seed(int(seed))
        shapes, sd = self.shapes(), {}
        for k in PARAM_KEYS:
            shape = shapes[k]
            w = torch.empty(*shape, dtype=torch.float32, device=self.device)
            if k.endswith("embed.weight"):
                w.uniform_(0.0, 1.0, generator=gen)
            elif k.rsplit(".", 1)[0] in BN_NAMES:
                w.fill_(1.0 if k.endswith(".weight") else 0.0)
            else:
                fan_in = shapes[k.rsplit(".", 1)[0] + ".weight"][1]
                bound = 1.0 / math.sqrt(fan_in)
                w.uniform_(-bound, bound, generator=gen)
            sd[k] = w
        return sd

    # ---- one forward and backward pass ------------------------------------------------------------------------------------------
    def _upload(self, x_flat, y0, yhat, t, e):
        """check_step_args, then -- and only then -- the uploads: t as int32, the schedule coefficients of the batch gathered on the CPU."""
        B = check_step_args(x_flat, y0, yhat, t, e, self.D, self.C, self.T)
        dev = self.device
        ca = self.alphas_bar_sqrt[t].contiguous().to(dev)                # CPU gathers: t is known to lie in [0, T)
        cb = self.one_minus_alphas_bar_sqrt[t].contiguous().to(dev)
        t32 = t.to(torch.int32).to(dev)
        return B, x_flat.to(dev).contiguous(), y0.to(dev).contiguous(), yhat.to(dev).contiguous(), t32, e.to(dev).contiguous(), ca, cb

    def _grads(self, x_flat, y0, yhat, t, e, track: bool):
        """(loss, {key: gradient}) with the Linear weights' gradients as packed images; track: update the running statistics."""
        B, x, y0, yhat, t32, e, ca, cb = self._upload(x_flat, y0, yhat, t, e)
        p, buf, g = self.p, self.buf, {}
        stats = lambda name: dict(running_mean=buf[name + ".running_mean"], running_var=buf[name + ".running_var"]) if track else {}  # noqa: E731

        def bn(name, u, act, **kw):
            return ops.bn_train_forward(u, p[name + ".weight"], p[name + ".bias"], act=act, **kw, **stats(name))

        # the encoder (latent_model.py:127-135, 155, 170-171)
        u0 = ops.linear(x, p["encoder_x.0.weight"], p["encoder_x.0.bias"])
        h0, xh0, rs0 = bn("encoder_x.1", u0, "softplus")
        u1 = ops.linear(h0, p["encoder_x.3.weight"], p["encoder_x.3.bias"])
        h1, xh1, rs1 = bn("encoder_x.4", u1, "softplus")
        u2 = ops.linear(h1, p["encoder_x.6.weight"], p["encoder_x.6.bias"])
        xe, xh2, rs2 = bn("norm", u2, None)
        # the trunk (:172-184)
        yt = ops.qsample(y0, yhat, e, ca, cb)
        inp = torch.cat([yt, yhat, torch.zeros(B, LIN1_K - 2 * self.C, dtype=torch.float32, device=self.device)], dim=1).contiguous()
        v1 = ops.linear(inp, p["lin1.lin.weight"], p["lin1.lin.bias"])
        y1, xh3, rs3 = bn("unetnorm1", v1, "softplus", table=p["lin1.embed.weight"], t=t32, mul=xe)
        v2 = ops.linear(y1, p["lin2.lin.weight"], p["lin2.lin.bias"])
        y2, xh4, rs4 = bn("unetnorm2", v2, "softplus", table=p["lin2.embed.weight"], t=t32)
        v3 = ops.linear(y2, p["lin3.lin.weight"], p["lin3.lin.bias"])
        y3, xh5, rs5 = bn("unetnorm3", v3, "softplus", table=p["lin3.embed.weight"], t=t32)
        out = ops.linear(y3, p["lin4.weight"], p["lin4.bias"])
        loss, dout = ops.mse_grad(out, e)

        def bn_back(name, d, xh, rs, act, **kw):
            r = ops.bn_train_backward(d, xh, rs, p[name + ".weight"], p[name + ".bias"], act=act, **kw)
            g[name + ".weight"], g[name + ".bias"] = r["dgamma"], r["dbeta"]
            return r

        # the gradients at the activations: every read of a weight by the backward chain
        r5 = bn_back("unetnorm3", ops.linear_grad_input(dout, p["lin4.weight"]), xh5, rs5, "softplus", u=v3, table=p["lin3.embed.weight"], t=t32)
        r4 = bn_back("unetnorm2", ops.linear_grad_input(r5["du"], p["lin3.lin.weight"]), xh4, rs4, "softplus", u=v2,
                     table=p["lin2.embed.weight"], t=t32)
        r3 = bn_back("unetnorm1", ops.linear_grad_input(r4["du"], p["lin2.lin.weight"]), xh3, rs3, "softplus", u=v1,
                     table=p["lin1.embed.weight"], t=t32, mul=xe, want_dmul=True)
        r2 = bn_back("norm", r3["dmul"], xh2, rs2, None)
        r1 = bn_back("encoder_x.4", ops.linear_grad_input(r2["du"], p["encoder_x.6.weight"]), xh1, rs1, "softplus")
        r0 = bn_back("encoder_x.1", ops.linear_grad_input(r1["du"], p["encoder_x.3.weight"]), xh0, rs0, "softplus")
        g["lin3.embed.weight"], g["lin2.embed.weight"], g["lin1.embed.weight"] = r5["dtable"], r4["dtable"], r3["dtable"]
        # the gradients at the Linear layers' parameters (gradient-only mode: dout already carries the mean's 2 / (B C))
        for key, dy, a in (("encoder_x.0", r0["du"], x), ("encoder_x.3", r1["du"], h0), ("encoder_x.6", r2["du"], h1), ("lin1.lin", r3["du"], inp),
                           ("lin2.lin", r4["du"], y1), ("lin3.lin", r5["du"], y2), ("lin4", dout, y3)):
            g[key + ".weight"] = ops.linear_wgrad_adam(dy, a, p[key + ".weight"], None, None, None, return_grad=True)
            g[key + ".bias"] = ops.bias_grad_adam(dy, None, None, None, None, return_grad=True)
        return loss, g

    def gradients(self, x_flat, y0, yhat, t, e) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
        """(loss, {reference key: gradient}) of one batch, materialised and unclipped, in the reference's shapes (lin1's padding cut off).
        Changes no state: the running statistics are left alone."""
        loss, g = self._grads(x_flat, y0, yhat, t, e, track=False)
        out = {k: (g[k].unpack() if isinstance(g[k], ops.PackedWeight) else g[k]) for k in PARAM_KEYS}
        out["lin1.lin.weight"] = out["lin1.lin.weight"][:, :2 * self.C].contiguous()
        return loss, out

    def step(self, x_flat, y0, yhat, t, e) -> Tuple[torch.Tensor, torch.Tensor]:
        """One optimizer step on a batch: (loss, total_norm), both device scalars of the pass BEFORE the update (total_norm: the gradient
        norm clip_grad_norm_ returns).  x_flat [B, D], y0 (one-hot) / yhat (the conditioner's softmax) / e (the noise) [B, C], t [B] int64
        on the CPU; 2 <= B <= 128."""
        loss, g = self._grads(x_flat, y0, yhat, t, e, track=True)
        # every read of a weight is behind us (same stream): the in-place updates may run
        acc = torch.empty((), dtype=torch.float32, device=self.device)
        for i, k in enumerate(PARAM_KEYS):
            ops.sumsq(g[k], acc, accumulate=i > 0)
        a = ops.adam_step(self.lr, self.t + 1, betas=self.betas, eps=self.eps)
        if self.shadow is None:
            for k in PARAM_KEYS:
                ops.clip_adam(self.p[k], self.m[k], self.v[k], g[k], a, sumsq=acc, max_norm=self.grad_clip)
        else:                                                # EMA.update after optimizer.step() (:1006-1011), in the optimizer's own pass
            e = ops.ema_step(self.ema_rate)
            for k in PARAM_KEYS:
                ops.clip_adam(self.p[k], self.m[k], self.v[k], g[k], a, sumsq=acc, max_norm=self.grad_clip, shadow=self.shadow[k], ema=e)
        self.t += 1                                          # counted once all 29 updates are enqueued
        self.batches_tracked += 1
        self.last_sumsq = acc
        return loss, torch.sqrt(acc)

    # ---- state ------------------------------------------------------------------------------------------------------------------
    def tensors(self, which: str = "p") -> Dict[str, torch.Tensor]:
        """The parameters ('p'), Adam's moments ('m', 'v') or the EMA shadow ('ema', with a rate only) as row-major device tensors,
        lin1.lin.weight WITH its padded columns."""
        if which == "ema" and self.shadow is None:
            raise ValueError("this trainer keeps no EMA shadow (ema_rate=None)")
        src = {"p": self.p, "m": self.m, "v": self.v, "ema": self.shadow}[which]
        return {k: (q.unpack() if isinstance(q, ops.PackedWeight) else q.clone()) for k, q in src.items()}

    def state_dict(self, cpu: bool = True) -> Dict[str, torch.Tensor]:
        """ConditionalModel.state_dict(): the reference's keys and shapes, the running statistics and num_batches_tracked (int64)
        included -- what load_noise_estimators / EnsembleEngine.load_member read.  cpu=False keeps the tensors on the device."""
        return self._state_dict("p", cpu)

    def ema_state_dict(self, cpu: bool = True) -> Dict[str, torch.Tensor]:
        """What the reference's EMA.ema(model); model.state_dict() gives (:1498-1502): state_dict()'s keys, shapes and dtypes with the
        SHADOW under the 29 parameter keys, and the LIVE running statistics and num_batches_tracked -- the reference's EMA walks
        named_parameters() only, so the buffers are the model's own.  Needs a trainer built with ema_rate."""
        if self.shadow is None:
            raise ValueError("this trainer keeps no EMA shadow (ema_rate=None)")
        return self._state_dict("ema", cpu)

    def _state_dict(self, which: str, cpu: bool) -> Dict[str, torch.Tensor]:
        full = self.tensors(which)
        full["lin1.lin.weight"] = full["lin1.lin.weight"][:, :2 * self.C].contiguous()
        sd: Dict[str, torch.Tensor] = {}
        for k in PARAM_KEYS:
            sd[k] = full[k]
            name = k.rsplit(".", 1)[0]
            if k.endswith(".bias") and name in BN_NAMES:
                sd[name + ".running_mean"] = self.buf[name + ".running_mean"].clone()
                sd[name + ".running_var"] = self.buf[name + ".running_var"].clone()
                sd[name + ".num_batches_tracked"] = torch.tensor(self.batches_tracked, dtype=torch.int64)
        return {k: (v.detach().cpu() if cpu else v.detach().to(self.device)) for k, v in sd.items()}

    # ---- the whole training state, for snapshots (snapshot.py) ---------------------------------------------------------------------
    def _meta(self) -> dict:
        ema = {} if self.ema_rate is None else {"ema_rate": self.ema_rate}
        return dict({"format": snapshot.FORMAT, "kind": "noise_estimator", "num_classes": self.C, "data_dim": self.D, "hidden_dim": self.H,
                     "feature_dim": self.F, "timesteps": self.T}, **ema, **self.run_meta)

    def _state_parts(self):
        """(name in a snapshot, the dict of this trainer) of everything stored under the parameters' keys"""
        parts = (("p", self.p), ("m", self.m), ("v", self.v))
        return parts if self.shadow is None else parts + (("ema", self.shadow),)

    def training_state(self) -> dict:
        """Everything a continued run needs, on the CPU, row-major, in the reference's keys and shapes: {'meta', 'p', 'm', 'v' (Adam's
        moments under the parameters' keys; lin1.lin.weight cut to [F, 2C] in all three), 'buf' (the running statistics), 't',
        'batches_tracked', 'lr'}, and with an EMA rate 'ema' (the shadow, keys and shapes as 'p') and meta's 'ema_rate'.  One tensor
        is unpacked, copied out and released at a time: the device holds at most one row-major weight beside the model."""
        def out(k, q):
            w = q.unpack() if isinstance(q, ops.PackedWeight) else q
            if k == "lin1.lin.weight":
                w = w[:, :2 * self.C]
            return w.detach().contiguous().cpu()

        state = {"meta": self._meta()}
        for which, src in self._state_parts():
            state[which] = {k: out(k, src[k]) for k in PARAM_KEYS}
        state["buf"] = {k: b.detach().cpu().clone() for k, b in self.buf.items()}
        state.update(t=int(self.t), batches_tracked=int(self.batches_tracked), lr=float(self.lr))
        return state

    def load_training_state(self, state: dict) -> None:
        """training_state() of a run with this run's meta (snapshot.check_meta: a ValueError names the field that differs), put back
        bit for bit: the packed images are rebuilt from the row-major tensors (PackedWeight: padding rows zero, as they were), one tensor
        at a time.  Everything is checked before the first tensor of this trainer is replaced.  The EMA shadow must be kept on both sides or
        on neither, at one rate: a ValueError names ema_rate otherwise."""
        snapshot.check_meta(state.get("meta"), self._meta())
        if self.ema_rate is None and "ema" in state:         # check_meta has refused a snapshot that records a rate; this one only holds a shadow
            raise ValueError("ema_rate: the snapshot holds an EMA shadow ('ema'), this run keeps none (ema_rate=None)")
        if self.ema_rate is not None and "ema" not in state:
            raise ValueError("ema_rate: the snapshot records a rate and holds no 'ema' entry")
        shapes = self.shapes()
        for which, _ in self._state_parts():
            for k in PARAM_KEYS:
                if k not in state[which]:
                    raise KeyError(f"the snapshot's '{which}' is missing '{k}'")
                if tuple(state[which][k].shape) != shapes[k]:
                    raise ValueError(f"{which}['{k}'] has shape {tuple(state[which][k].shape)}, expected {shapes[k]}")
        for k, b in self.buf.items():
            if k not in state["buf"] or tuple(state["buf"][k].shape) != tuple(b.shape):
                raise ValueError(f"buf['{k}'] is missing or has another shape than {tuple(b.shape)}")
        for which, dst in self._state_parts():
            for k in PARAM_KEYS:
                w = state[which][k].detach().to(self.device, torch.float32).contiguous()
                if k == "lin1.lin.weight":
                    w = pad_lin1(w)
                if k in PACKED_KEYS:
                    dst[k] = None                            # the old image goes before the new one is built
                    dst[k] = ops.PackedWeight(w)
                else:
                    dst[k].copy_(w)
                del w
        for k, b in self.buf.items():
            b.copy_(state["buf"][k])
        self.t, self.batches_tracked, self.lr = int(state["t"]), int(state["batches_tracked"]), float(state["lr"])


# ---- the training loop of one noise estimator (Diffusion.train, :842-1141) ---------------------------------------------------------------
def train_request(args, config, mlp_idx: int, n_mlps: int, operand_dtype: str) -> dict:
    """Everything train_noise_estimator refuses, before anything is built: an mlp_idx outside -1 (the noise estimator conditioned on the
    full ViT's output) .. n_mlps - 1 (on that mapping MLP), more than one GPU, --train_guidance_only, another conditioner than 'sevit',
    the fp16 mode; with args.resume_training a missing <log_path>/ckpt.pth (FileNotFoundError, so a missing file costs nothing); with
    args.ema (main --ema) a config.model.ema_rate that is missing or outside (0, 1), refused by name.  Returns the run's settings:
    {'mlp_idx', 'snap_path', 'snapshot_epochs', 'resume', 'ema_rate' (None without --ema, whatever model.ema says in the config)}."""
    if not -1 <= mlp_idx < n_mlps:
        raise NotImplementedError(f"mlp_idx must be -1 (the ViT's output) or in [0, {n_mlps}) (mlp_idx={mlp_idx})")
    _, world = nd_dist.rank_world()
    if world > 1:
        raise NotImplementedError("Diffusion.train runs on one GPU: world size > 1 is not implemented")
    if getattr(args, "train_guidance_only", False):
        raise NotImplementedError("--train_guidance_only is not implemented")
    if config.diffusion.aux_cls.arch != "sevit":
        raise NotImplementedError(f"aux_cls.arch == {config.diffusion.aux_cls.arch!r}: only 'sevit' is implemented")
    if operand_dtype != "f32":
        raise NotImplementedError("training runs in fp32 mode: the fp16 mode is not implemented")
    snap_path = os.path.join(args.log_path, "ckpt.pth")                   # the reference's file name (:890-908, commented out there)
    resume = bool(getattr(args, "resume_training", False))
    if resume:
        snapshot.require(snap_path)
    ema_rate = None
    if getattr(args, "ema", False):
        ema_rate = getattr(config.model, "ema_rate", None)
        if isinstance(ema_rate, bool) or not isinstance(ema_rate, (int, float)) or not 0.0 < float(ema_rate) < 1.0:
            raise ValueError(f"model.ema_rate: --ema needs a rate in (0, 1) in the config (model.ema_rate={ema_rate!r})")
    return {"mlp_idx": mlp_idx, "snap_path": snap_path, "snapshot_epochs": int(getattr(args, "snapshot_epochs", 0) or 0), "resume": resume,
            "ema_rate": ema_rate}


def default_loader(args, config, device, split: str, batch_size: int, **order):
    """data.split_loader of <dataroot>/<split> as the run's flags ask for it: a DataLoader with config.data.num_workers processes, or
    with --train_cache device the same batches in the same order from data.DeviceImageSet, decoded once and gathered on the GPU
    (--cache_dir keeps the decoded sets for later runs)."""
    side = int(round((config.model.data_dim / 3) ** 0.5))          # 224 for data_dim = 150528 (3 x 224 x 224)
    size = (side, side) if 3 * side * side == config.model.data_dim else (224, 224)
    return split_loader(config.data.dataroot, split, config.data.dataset, args.preprocess, size, batch_size,
                        cache=getattr(args, "train_cache", None) or "none", flag="train_cache", cache_dir=getattr(args, "cache_dir", None),
                        device=device, num_workers=int(getattr(config.data, "num_workers", 0) or 0), **order)


def validate(engine: EnsembleEngine, trainer: NoiseEstimatorTrainer, valid_loader, yhat_of, num_timesteps: int) -> float:
    """The validation set sampled with the current LIVE weights on the FULL chain, with or without --sample_steps (p_sample_loop in eval
    mode: trainer.state_dict() loaded into the one-member `engine`, noise drawn in the library): the top-1 accuracy of y_0 in %, averaged
    over the batches (:1103-1110)."""
    engine.load_member(0, trainer.state_dict(cpu=False))
    acc_sum, n_batches = 0.0, 0
    for images_raw, target in valid_loader:
        images = images_raw.to(trainer.device, torch.float32).contiguous()
        yhat = yhat_of(images)
        engine.encode(torch.flatten(images, 1))
        y_0 = engine.sample(yhat[None], yhat[None], None, mc=1, T=num_timesteps, use_graph=False)[0]   # :1103-1108
        acc_sum += float((y_0.argmax(dim=1).cpu() == target.cpu()).float().mean()) * 100.0    # accuracy in %, :1110
        n_batches += 1
    if n_batches == 0:
        raise ValueError("the validation loader is empty")
    return acc_sum / n_batches


def save_best(trainer: NoiseEstimatorTrainer, log_path: str, mlp_idx: int, epoch: int, acc: float) -> str:
    """<log_path>/diffu{idx}_ckpt_best_eph{epoch}_acc{acc:.4f}.pth = {'noise_estimator', 'optimizer', 'epoch'}, the layout
    load_noise_estimators reads.  'optimizer' holds {'step', 'lr'} only: the best file is for inference, and Adam's moments of the
    150528 x 4096 layer would triple it (the whole training state goes to ckpt.pth instead).  A trainer that keeps an EMA shadow adds a
    fourth entry 'ema' = trainer.ema_state_dict(), what --use_ema reads.  Returns the path."""
    states = {'noise_estimator': trainer.state_dict(), 'optimizer': {'step': trainer.t, 'lr': trainer.lr}, 'epoch': epoch}
    if trainer.ema_rate is not None:
        states['ema'] = trainer.ema_state_dict()
    best = os.path.join(log_path, "diffu{}_ckpt_best_eph{}_acc{:.4f}.pth".format(mlp_idx, epoch, acc))
    torch.save(states, best)
    print("Saved diffusion model {} at {}".format(mlp_idx, best))
    return best


def train_noise_estimator(request: dict, args, config, device, *, guide, alphas, one_minus_alphas_bar_sqrt, seed: int, train_loader=None,
                          valid_loader=None, built=None) -> dict:
    """Diffusion.train (:842-1141) for the noise estimator of train_request's `request`, on ONE GPU.  A step: the learning rate of lr_at
    (when optim.lr_schedule is set), the antithetic timestep draw, the softmax of guide(images, include_full_vit)[mlp_idx] (the runner's
    compute_guiding_prediction) as yhat, e = randn, and one NoiseEstimatorTrainer.step.  Every training.validation_freq epochs and on
    the last one: validate, and on a new best accuracy save_best; validation and the choice of the best epoch stay on the live weights
    with --ema too, as in the reference, so the losses, accuracies, best epochs and 'noise_estimator' bits are those of a run without
    the flag, while every step's optimizer pass updates the shadow, ckpt.pth carries it and a resumed run restores it.
    The whole training state goes to <log_path>/ckpt.pth (the reference's name, :890-908) every args.snapshot_epochs epochs and after
    the last (snapshot.save_run): 'loop' = {'next_epoch', 'step', 'max_accuracy', 'best', 'losses', 'accuracies'}, 'rng' with the
    validation engine's sampler state; args.resume_training continues from it at the top of epoch 'next_epoch', with lr_at on the true
    epoch index, and returns the earlier epochs too.
    train_loader / valid_loader: loaders of (images [B, 3, S, S], labels [B]) batches (default: default_loader of 'training', shuffled in
    batches of training.batch_size, and of 'validation' in batches of testing.batch_size, drop_last).  built(trainer) is called as soon
    as the trainer exists: it stays reachable when the run is cut.
    Returns {'losses': per-epoch last loss, 'accuracies': {epoch: acc}, 'best': path or None}."""
    mlp_idx, snap_path, num_timesteps = request["mlp_idx"], request["snap_path"], config.diffusion.timesteps
    print('NOTE: TRAINING DIFFUSION MODEL FOR MLP {}'.format(mlp_idx) if mlp_idx >= 0 else 'NOTE: TRAINING DIFFUSION MODEL FOR ViT OUTPUT')
    B_valid = config.testing.batch_size
    if train_loader is None:
        train_loader = default_loader(args, config, device, "training", config.training.batch_size, shuffle=True)
    if valid_loader is None:
        valid_loader = default_loader(args, config, device, "validation", B_valid, shuffle=False, drop_last=True)
    trainer = NoiseEstimatorTrainer(config, device, seed=seed, ema_rate=request["ema_rate"])
    if built is not None:
        built(trainer)
    batch_size = snapshot.loader_batch_size(train_loader)
    trainer.run_meta = {"mlp_idx": int(mlp_idx), "dataset": config.data.dataset, "train_batches": len(train_loader),
                        "batch_size": config.training.batch_size if batch_size is None else batch_size,
                        "epochs": int(config.training.n_epochs)}
    engine: Optional[EnsembleEngine] = None
    n_epochs, freq = config.training.n_epochs, config.training.validation_freq
    log_freq = getattr(config.training, "logging_freq", 0) or 0
    max_accuracy, step, best, first_epoch = 0.0, 0, None, 0
    losses, accuracies = [], {}

    def yhat_of(images):
        logits = guide(images, include_full_vit=mlp_idx == -1)
        return ops.softmax_rows(logits[mlp_idx].contiguous())            # :955-958

    def validation_engine():
        eng = EnsembleEngine(config.data.num_classes, config.model.data_dim, config.model.hidden_dim, config.model.feature_dim,
                             num_timesteps, n_members=1, max_batch=B_valid, max_rows=B_valid, device=device)
        eng.set_schedule(alphas, one_minus_alphas_bar_sqrt)
        eng.seed(seed)
        return eng

    if request["resume"]:
        snap = snapshot.load_run(snap_path, trainer)
        loop = snap["loop"]
        first_epoch, step, max_accuracy, best = int(loop["next_epoch"]), int(loop["step"]), float(loop["max_accuracy"]), loop["best"]
        losses, accuracies = [float(v) for v in loop["losses"]], {int(k): float(v) for k, v in loop["accuracies"].items()}
        if snap["rng"].get("engine") is not None:                        # the run had validated: its sampler state goes back
            engine = validation_engine()
        snapshot.set_rng_state(snap["rng"], device, train_loader, engine)
        del snap
        logging.info(f"Resumed from {snap_path} at epoch {first_epoch}, step {step}")
    for epoch in range(first_epoch, n_epochs):
        loss = None
        for i, (x_raw, labels) in enumerate(train_loader):
            x = x_raw.to(device, torch.float32).contiguous()
            y0, _ = cast_label_to_one_hot_and_prototype(labels, config, return_prototype=False)
            if config.optim.lr_schedule:
                trainer.lr = lr_at(i / len(train_loader) + epoch, config)     # :927-928
            n = x.shape[0]
            step += 1
            t = antithetic_timesteps(n, num_timesteps)                        # :945-948, on the CPU
            yhat = yhat_of(x)
            e = torch.randn(n, config.data.num_classes, dtype=torch.float32, device=device)    # :965
            loss, _ = trainer.step(torch.flatten(x, 1), y0.to(device), yhat, t, e)
            if log_freq and (step % log_freq == 0 or step == 1):
                logging.info(f"During epoch: {epoch}, step: {step}, Noise Estimation loss: {loss.item()}")
        if loss is None:
            raise ValueError("the training loader is empty")
        losses.append(float(loss))
        logging.info(f"epoch: {epoch}, step: {step}, Noise Estimation loss: {losses[-1]}")
        if epoch % freq == 0 or epoch + 1 == n_epochs:                        # :1054-1055
            if engine is None:
                engine = validation_engine()
            acc_avg = validate(engine, trainer, valid_loader, yhat_of, num_timesteps)
            accuracies[epoch] = acc_avg
            if acc_avg > max_accuracy:
                logging.info("Update accuracy at Epoch {}.".format(epoch))
                best = save_best(trainer, args.log_path, mlp_idx, epoch, acc_avg)
            max_accuracy = max(max_accuracy, acc_avg)
            logging.info(f"epoch: {epoch}, step: {step}, Average diffusion {mlp_idx} accuracy: {acc_avg}%, "
                         f"Max diffusion {mlp_idx} accuracy: {max_accuracy:.2f}%, ")
        if snapshot.due(epoch, n_epochs, request["snapshot_epochs"]):
            loop = {"next_epoch": epoch + 1, "step": step, "max_accuracy": max_accuracy, "best": best, "losses": list(losses),
                    "accuracies": dict(accuracies)}
            snapshot.save_run(snap_path, trainer, loop, device, train_loader, engine)
    return {"losses": losses, "accuracies": accuracies, "best": best}
