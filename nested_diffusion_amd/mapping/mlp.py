"""The mapping MLP: mapping/models/mlp.py::Classifier over a state_dict, its forward and its input gradient."""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

from .. import ops


class Classifier:
    """mapping/models/mlp.py:4-29.  forward: reshape(-1, in_features) -> 3x (Linear, ReLU) -> Linear.
    (dropout is declared by the reference but never applied in forward.)"""

    KEYS = [f"linear{i}.{s}" for i in range(1, 5) for s in ("weight", "bias")]

    def __init__(self, state_dict: Dict[str, torch.Tensor], device="cuda", dtype="f32"):
        missing = [k for k in self.KEYS if k not in state_dict]
        if missing:
            raise KeyError(f"Classifier state_dict is missing {missing}")
        self.device = torch.device(device)
        self.in_features = state_dict["linear1.weight"].shape[1]
        self.p = {}
        for k in self.KEYS:
            t = state_dict[k].detach().to(self.device, torch.float32).contiguous()
            # weights are repacked once into the streaming kernels' fragment order; the row-major copy is dropped
            self.p[k] = ops.PackedWeight(t, dtype) if k.endswith("weight") else t

    def __call__(self, x: torch.Tensor, dataset: str = "any") -> torch.Tensor:
        return self.forward(x, dataset)

    def forward(self, x: torch.Tensor, dataset: str = "any") -> torch.Tensor:
        return self.forward_recorded(x)[0]

    def forward_recorded(self, x: torch.Tensor) -> Tuple[torch.Tensor, List[torch.Tensor]]:
        """The four launches of the forward, keeping the three post-ReLU activations input_grad gates with: (logits, [h1, h2, h3])."""
        p, h, acts = self.p, x.reshape(-1, self.in_features), []
        for i in (1, 2, 3):
            h = ops.linear(h, p[f"linear{i}.weight"], p[f"linear{i}.bias"], act="relu")
            acts.append(h)
        return ops.linear(h, p["linear4.weight"], p["linear4.bias"]), acts

    def input_grad(self, dlogits: torch.Tensor, acts: List[torch.Tensor], add: Optional[torch.Tensor] = None) -> torch.Tensor:
        """dL/d(the MLP's input) [B, in_features] from dlogits [B, C]: four linear_grad_input calls down the layers, each gated by the
        activation forward_recorded kept; `add` [B, in_features] joins at the input (the gradient the shared ViT prefix already carries)."""
        p = self.p
        d = ops.linear_grad_input(dlogits, p["linear4.weight"], gate=acts[2])
        d = ops.linear_grad_input(d, p["linear3.weight"], gate=acts[1])
        d = ops.linear_grad_input(d, p["linear2.weight"], gate=acts[0])
        return ops.linear_grad_input(d, p["linear1.weight"], add=add)
