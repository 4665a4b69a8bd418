"""Drop-in mirror of the reference's diffusion/latent_model.py for arch == 'linear':
ConditionalLinear and ConditionalModel with the reference's parameter names (so
`load_state_dict(state['noise_estimator'])` of a reference checkpoint works unchanged) and a
forward() that runs in libnd_hip.so.  Inference only: eval mode, no autograd.

The other encoders of the reference file (NewClassifier, SimNet, FashionCNN, ResNetEncoder, LeNet,
LeNet5; latent_model.py:50-90, 216-368) are never instantiated by the shipped configs
(configs/*.yml:18 `arch: linear`) and are out of scope.
"""
from __future__ import annotations

import weakref
from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib
from .engine import EnsembleEngine


# ---- the layout of ConditionalModel(guidance=True, arch 'linear'), for everything that holds one without the nn.Module -----------------
LIN1_K = 16     # lin1.lin.weight [F, 2C] is held padded to 16 columns wherever it is a packed image: those want K % 16 == 0


def member_shapes(C: int, D: int, H: int, F: int, T: int) -> Dict[str, Tuple[int, ...]]:
    """The reference's parameter shapes (latent_model.py:108-167; embedding tables of T + 1 rows), in registration order."""
    s: Dict[str, Tuple[int, ...]] = {}
    for name, n_in, n_out, after in (("encoder_x.0", D, H, "encoder_x.1"), ("encoder_x.3", H, H, "encoder_x.4"), ("encoder_x.6", H, F, "norm"),
                                     ("lin1.lin", 2 * C, F, "unetnorm1"), ("lin2.lin", F, F, "unetnorm2"), ("lin3.lin", F, F, "unetnorm3"),
                                     ("lin4", F, C, None)):
        s[name + ".weight"], s[name + ".bias"] = (n_out, n_in), (n_out,)             # a Linear
        if name.endswith(".lin"):
            s[name[:-4] + ".embed.weight"] = (T + 1, F)                               # ConditionalLinear's per-timestep gain
        if after:
            s[after + ".weight"] = s[after + ".bias"] = (n_out,)                      # the BatchNorm1d behind it
    return s


def check_member_dims(C: int, D: int, H: int, F: int, T: int) -> None:
    """What the packed images and the kernels behind them take: D, H, F positive multiples of 16, 1 <= 2C <= LIN1_K, T >= 1."""
    if min(D, H, F) < 16 or D % 16 or H % 16 or F % 16:
        raise ValueError(f"data_dim, hidden_dim and feature_dim must be positive multiples of 16 (D={D}, H={H}, F={F})")
    if not 1 <= 2 * C <= LIN1_K:
        raise ValueError(f"num_classes must lie in [1, {LIN1_K // 2}] (num_classes={C})")
    if T < 1:
        raise ValueError(f"diffusion.timesteps must be at least 1: the embedding tables must have T + 1 >= 2 rows (T={T})")


def pad_lin1(w: torch.Tensor) -> torch.Tensor:
    """lin1.lin.weight [F, 2C] -> [F, LIN1_K]: the input first, the new columns +0.0 (the trainer's gradient there is exactly +0)."""
    return torch.cat([w, torch.zeros(w.shape[0], LIN1_K - w.shape[1], dtype=w.dtype, device=w.device)], dim=1).contiguous()


class _TensorKey:
    """Identity of a tensor's CONTENTS for the two caches below, in a form the caching allocator cannot forge.

    (data_ptr, _version, shape) alone is not enough: a NEW tensor placed at the freed address of the previous one (same
    shape, _version 0) -- `x = img.cuda().flatten(1)` per batch, or any loop that drops the old batch before it builds the next --
    carries the same triple.  The key therefore also holds a weak reference to the tensor's untyped storage object (torch keeps
    ONE Python object per live storage): a storage that has been freed is a dead reference, a recycled address is a different
    object, and both read as "changed".  Views of one storage share it and share its version counter, so re-flattening the
    same batch still hits."""

    __slots__ = ("storage", "meta")

    def __init__(self, t: torch.Tensor):
        self.storage = weakref.ref(t.untyped_storage())
        self.meta = (t.data_ptr(), t._version, tuple(t.shape), tuple(t.stride()), t.dtype, str(t.device))

    def matches(self, t: torch.Tensor) -> bool:
        alive = self.storage()
        return (alive is not None and alive is t.untyped_storage()
                and self.meta == (t.data_ptr(), t._version, tuple(t.shape), tuple(t.stride()), t.dtype, str(t.device)))


class ConditionalLinear(nn.Module):
    """latent_model.py:93-105: parameter container (lin: Linear, embed: Embedding(n_steps, num_out))."""

    def __init__(self, num_in, num_out, n_steps):
        super().__init__()
        self.num_out = num_out
        self.lin = nn.Linear(num_in, num_out)
        self.embed = nn.Embedding(n_steps, num_out)
        self.embed.weight.data.uniform_()

    def forward(self, x, t):
        raise _lib.NdError("ConditionalLinear runs fused inside ConditionalModel.forward (libnd_hip.so)")


class ConditionalModel(nn.Module):
    """latent_model.py:108-184 with arch 'linear'.  `config` needs .diffusion.timesteps,
    .model.{data_dim, arch, feature_dim, hidden_dim}, .data.{num_classes, dataset}."""

    def __init__(self, config, guidance=False, max_batch: int = 128, max_rows: Optional[int] = None):
        super().__init__()
        n_steps = config.diffusion.timesteps + 1
        data_dim = config.model.data_dim
        y_dim = config.data.num_classes
        arch = config.model.arch
        feature_dim = config.model.feature_dim
        hidden_dim = config.model.hidden_dim
        if arch != "linear":
            raise NotImplementedError(f"arch '{arch}': only 'linear' (the shipped configs) is on the hot path")
        self.guidance = guidance
        self.dims = (y_dim, data_dim, hidden_dim, feature_dim, config.diffusion.timesteps)
        self.max_batch, self.max_rows = max_batch, max_rows or max_batch
        self.encoder_x = nn.Sequential(
            nn.Linear(data_dim, hidden_dim), nn.BatchNorm1d(hidden_dim), nn.Softplus(),
            nn.Linear(hidden_dim, hidden_dim), nn.BatchNorm1d(hidden_dim), nn.Softplus(),
            nn.Linear(hidden_dim, feature_dim))
        self.norm = nn.BatchNorm1d(feature_dim)
        self.lin1 = ConditionalLinear(y_dim * 2 if guidance else y_dim, feature_dim, n_steps)   # latent_model.py:155-158
        self.unetnorm1 = nn.BatchNorm1d(feature_dim)
        self.lin2 = ConditionalLinear(feature_dim, feature_dim, n_steps)
        self.unetnorm2 = nn.BatchNorm1d(feature_dim)
        self.lin3 = ConditionalLinear(feature_dim, feature_dim, n_steps)
        self.unetnorm3 = nn.BatchNorm1d(feature_dim)
        self.lin4 = nn.Linear(feature_dim, y_dim)
        self._engine: Optional[EnsembleEngine] = None
        self._engine_sig = None
        self._enc_sig = None

    # -- HIP engine, rebuilt when the parameters move or change --------------------------------
    def _tensors(self):
        return list(self.parameters()) + list(self.buffers())

    def _signature_matches(self) -> bool:
        ts = self._tensors()
        return (self._engine_sig is not None and len(ts) == len(self._engine_sig)
                and all(k.matches(t) for k, t in zip(self._engine_sig, ts)))

    def hip_engine(self) -> EnsembleEngine:
        if self.training:
            raise _lib.NdError("ConditionalModel is inference-only here: call .eval() (BatchNorm uses running stats)")
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise _lib.NdError("ConditionalModel.forward needs the parameters on the GPU (.to('cuda')); no CPU fallback")
        if self._engine is None or not self._signature_matches():
            C, D, H, F, T = self.dims
            if self._engine is None or self._engine.device != dev:
                self._engine = EnsembleEngine(C, D, H, F, T, n_members=1, max_batch=self.max_batch, max_rows=self.max_rows,
                                              device=dev)
            self._engine.load_member(0, self.state_dict())      # [F, C] lin1 of guidance=False is widened there
            self._engine_sig, self._enc_sig = [_TensorKey(t) for t in self._tensors()], None
        return self._engine

    def encode(self, x: torch.Tensor) -> None:
        """xe = norm(encoder_x(x)) (latent_model.py:170-171: evaluated on every call there), cached here while `x` is provably
        the tensor contents of the last call (_TensorKey: live storage object + address + version counter + geometry), so the T
        calls of a p_sample_loop and the mc_trials loops over one batch (classification_train_separately.py:770-777) encode once."""
        eng = self.hip_engine()
        if self._enc_sig is None or not self._enc_sig.matches(x):
            self._enc_sig = None            # a failed encode must not leave a stale key behind
            eng.encode(x)
            self._enc_sig = _TensorKey(x)

    def forward(self, x, y, t, yhat=None):
        """eps_theta(x, y_t, t, yhat) -> [B, C] (latent_model.py:169-184)."""
        if self.guidance and yhat is None:
            raise ValueError("guidance=True requires yhat")
        if not self.guidance:
            yhat = torch.zeros_like(y)                          # ignored by the reference (latent_model.py:172): zero weights here
        t = torch.as_tensor(t).reshape(-1).cpu()
        if t.numel() not in (1, y.shape[0]):
            raise ValueError(f"t must hold 1 or {y.shape[0]} timesteps, got {t.numel()}")
        self.encode(x)
        eng = self.hip_engine()
        steps = torch.unique(t).tolist()
        if len(steps) == 1:                                     # the inference path: one t for the batch (diffusion_utils.py:68)
            return eng.eps_theta(0, y, yhat, int(steps[0]))
        # per-row timesteps (the training-time call shape, gamma = embed(t) per row, latent_model.py:101-105): rows are
        # independent, so evaluate the batch once per distinct t and keep each row from the pass of its own t
        out = None
        for step in steps:
            e = eng.eps_theta(0, y, yhat, int(step))
            out = e.clone() if out is None else torch.where((t == step).to(e.device)[:, None], e, out)
        return out
