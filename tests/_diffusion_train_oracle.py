"""TEST INFRASTRUCTURE ONLY: a torch-autograd restatement of one training step of the noise estimator
(diffusion/classification_train_separately.py:942-1006 on latent_model.py's ConditionalModel, guidance=True), in fp32 or fp64 on the CPU.
The forward is oracle.ref_cpu's (its Linear / ConditionalLinear helpers) with F.batch_norm(training=True) in place of the eval-mode
BatchNorm; backward is autograd, the clip is torch's clip_grad_norm_ and the optimizer torch.optim.Adam.  Pinned against the reference's
own five steps by tests/test_diffusion_train_oracle_host.py (tests/golden/diffusion_train.npz)."""
from __future__ import annotations

import os
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_cpu

BN_NAMES = ("encoder_x.1", "encoder_x.4", "norm", "unetnorm1", "unetnorm2", "unetnorm3")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "diffusion_train.npz")


def load_fixture() -> Dict[str, np.ndarray]:
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def fixture_state(fx: Dict[str, np.ndarray], prefix: str) -> Dict[str, torch.Tensor]:
    return {k[len(prefix):]: torch.from_numpy(v.copy()) for k, v in fx.items() if k.startswith(prefix)}


def random_state(D: int, H: int, Fd: int, C: int, T: int, seed: int) -> Dict[str, torch.Tensor]:
    """A fresh model's state dict: ref_cpu's initialiser with BatchNorm at its defaults (gamma 1, beta 0, rm 0, rv 1)."""
    return ref_cpu.init_cond_model_params(D, H, Fd, C, T, guidance=True, seed=seed, randomize_bn=False)


def random_batch(B: int, D: int, C: int, T: int, seed: int):
    """(x, y0, yhat, t, e) of one step: images in [0, 1), one-hot labels, a softmax, the antithetic timestep draw, the noise."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, D, generator=g)
    y0 = F.one_hot(torch.randint(0, C, (B,), generator=g), num_classes=C).float()
    yhat = torch.softmax(torch.randn(B, C, generator=g), dim=-1)
    t = torch.randint(low=0, high=T, size=(B // 2 + 1,), generator=g)
    t = torch.cat([t, T - 1 - t], dim=0)[:B]
    return x, y0, yhat, t, torch.randn(B, C, generator=g)


class Oracle:
    """The model's parameters as autograd leaves of `dtype`, torch.optim.Adam beside them."""

    def __init__(self, state: Dict[str, torch.Tensor], alphas_bar_sqrt: torch.Tensor, one_minus_alphas_bar_sqrt: torch.Tensor,
                 dtype=torch.float64, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, max_norm: float = 1.0):
        self.dtype, self.max_norm = dtype, max_norm
        self.p: Dict[str, torch.Tensor] = {}
        self.buf: Dict[str, torch.Tensor] = {}
        for k, v in state.items():
            if k.endswith("num_batches_tracked"):
                continue
            if k.endswith(("running_mean", "running_var")):
                self.buf[k] = v.detach().to(dtype).clone()
            else:
                self.p[k] = v.detach().to(dtype).clone().requires_grad_(True)
        self.ca, self.cb = alphas_bar_sqrt.to(dtype), one_minus_alphas_bar_sqrt.to(dtype)
        self.opt = torch.optim.Adam(list(self.p.values()), lr=lr, betas=betas, eps=eps)
        self.du: Dict[str, torch.Tensor] = {}

    def _forward(self, x, y_t, t, yhat, track: bool, keep: Optional[dict] = None):
        p = self.p

        def bn(u, name):
            rm, rv = (self.buf[name + ".running_mean"], self.buf[name + ".running_var"]) if track else (None, None)
            return F.batch_norm(u, rm, rv, p[name + ".weight"], p[name + ".bias"], True, 0.1, ref_cpu.BN_EPS)

        def lin(h, name):
            u = ref_cpu._big_linear(h, p[name + ".weight"], p[name + ".bias"])
            if keep is not None:
                u.retain_grad()
                keep[name] = u
            return u

        h = F.softplus(bn(lin(x, "encoder_x.0"), "encoder_x.1"))
        h = F.softplus(bn(lin(h, "encoder_x.3"), "encoder_x.4"))
        xe = bn(lin(h, "encoder_x.6"), "norm")
        y = torch.cat([y_t, yhat], dim=-1)
        y = F.softplus(bn(ref_cpu._cond_linear(p, "lin1", y, t), "unetnorm1")) * xe
        y = F.softplus(bn(ref_cpu._cond_linear(p, "lin2", y, t), "unetnorm2"))
        y = F.softplus(bn(ref_cpu._cond_linear(p, "lin3", y, t), "unetnorm3"))
        return F.linear(y, p["lin4.weight"], p["lin4.bias"])

    def backward(self, x, y0, yhat, t, e, track: bool = False) -> torch.Tensor:
        """The loss of one batch; the gradients are left in .grad of the leaves, dL/d(encoder Linear outputs) in self.du."""
        d = self.dtype
        x, y0, yhat, e = x.to(d), y0.to(d), yhat.to(d), e.to(d)
        a = self.ca[t][:, None]
        y_t = a * y0 + (1 - a) * yhat + self.cb[t][:, None] * e               # diffusion_utils.py:49
        keep: dict = {}
        loss = (e - self._forward(x, y_t, t, yhat, track, keep)).square().mean()
        self.opt.zero_grad()
        loss.backward()
        self.du = {k: u.grad.detach() for k, u in keep.items()}
        self.y_t = y_t.detach()
        return loss.detach()

    def grads(self) -> Dict[str, torch.Tensor]:
        return {k: v.grad.detach().clone() for k, v in self.p.items()}

    def step(self, x, y0, yhat, t, e):
        """(loss, total_norm) of one optimizer step, as the reference takes it."""
        loss = self.backward(x, y0, yhat, t, e, track=True)
        norm = torch.nn.utils.clip_grad_norm_(list(self.p.values()), self.max_norm)
        self.opt.step()
        return loss, norm.detach()

    def state(self) -> Dict[str, torch.Tensor]:
        out = {k: v.detach().clone() for k, v in self.p.items()}
        out.update({k: v.clone() for k, v in self.buf.items()})
        return out

    def eval_output(self, x, y, t: int, yhat) -> torch.Tensor:
        """The eval-mode forward (running statistics) at one timestep for every row."""
        d = self.dtype
        with torch.no_grad():
            tt = torch.full((x.shape[0],), int(t), dtype=torch.int64)
            return ref_cpu.cond_model_forward(self.state(), x.to(d), y.to(d), tt, yhat.to(d))


def fixture_run(fx: Dict[str, np.ndarray], dtype, prefix: str = "", steps: Optional[int] = None) -> dict:
    """The fixture's steps on the oracle in `dtype`: per-step loss and norm, the step-0 gradients, the final state, the eval output."""
    max_norm = 1e9 if prefix else 1.0
    o = Oracle(fixture_state(fx, "init/"), torch.from_numpy(fx["alphas_bar_sqrt"]), torch.from_numpy(fx["one_minus_alphas_bar_sqrt"]),
               dtype=dtype, max_norm=max_norm)
    C = int(fx["dims"][4])
    n = fx["x"].shape[0] if steps is None else steps
    res = {"loss": [], "norm": []}
    for s in range(n):
        x, yhat, e = (torch.from_numpy(fx[k][s]) for k in ("x", "yhat", "e"))
        t = torch.from_numpy(fx["t"][s])
        y0 = F.one_hot(torch.from_numpy(fx["labels"][s]), num_classes=C).float()
        if s == 0:
            o.backward(x, y0, yhat, t, e)
            res["grad0"] = o.grads()
        loss, norm = o.step(x, y0, yhat, t, e)
        res["loss"].append(float(loss))
        res["norm"].append(float(norm))
    res["final"] = o.state()
    res["eval_out"] = o.eval_output(x, torch.from_numpy(fx[prefix + "eval_y"]), int(fx["dims"][6]), yhat)
    return res
