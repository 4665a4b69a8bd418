"""Expectation over transformation (EOT) for attacks on a randomized defence: the gradient an attack follows is the mean over several
draws of the defence's randomness at the SAME point (Athalye et al., "Synthesizing robust adversarial examples"; autoattack's eot_iter,
which AutoAttack version='rand' sets to 20).

ensemble_grad.EnsembleTarget draws fresh sampler noise on every call, so an iterative attack on it averages over the randomness only
across its steps.  EOTTarget(model, n) wraps any model of the gradient attacks (a VisionTransformer, a mapping.ConditionerTarget, an
EnsembleTarget) and composes with every one of them -- attack.Attack, attack.L2Attack, autoattack.APGDAttack:

    input_grad(x, labels):  scores_k, g_k, loss_k = model.input_grad(x, labels)   for k = 1 .. n, in this order
                            grad = (((g_1 + g_2) + ...) + g_n) / n                (fp32, one add per draw and one true division; nd_eot_add)
                            return scores_n, grad, loss_n                         (the last draw's, as autoattack keeps them)

The first call's gradient tensor is the accumulator; n = 1 is a pure pass-through (no launch, the wrapped result itself).  The cost is
plain: every gradient of the attack becomes n gradients of the wrapped model.
"""
from __future__ import annotations

from typing import Tuple

import torch

from . import ops


class EOTTarget:
    """model with input_grad averaged over n draws: .device, forward(x) (one draw of the wrapped model) and input_grad(x, labels).  It
    has no attribute called `vit` (attack._vit would unwrap it); input_grad_margin (Carlini & Wagner) refuses by name.  Wrapping an
    EnsembleTarget advances its call counter by n per gradient."""

    def __init__(self, model, n: int):
        if isinstance(n, bool) or not isinstance(n, int):
            raise TypeError(f"EOTTarget needs an integer number of draws (n={n!r})")
        if n < 1:
            raise ValueError(f"EOTTarget needs at least one draw (n={n})")
        if not callable(getattr(model, "input_grad", None)):
            raise TypeError("EOTTarget wraps a model of the gradient attacks: it needs input_grad(x, labels)")
        self.model, self.n = model, n
        self.device = model.device

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.model.forward(x)

    __call__ = forward

    def input_grad(self, x: torch.Tensor, labels: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(scores, mean gradient, loss): the mean of n draws' gradients at x in call order, scores and loss of the last draw."""
        out = self.model.input_grad(x, labels)
        if self.n == 1:
            return out
        scores, acc, loss = out
        for k in range(2, self.n + 1):
            scores, g, loss = self.model.input_grad(x, labels)
            ops.eot_add(acc, g, self.n if k == self.n else 0)
        return scores, acc, loss

    def input_grad_margin(self, *args, **kwargs):
        raise NotImplementedError("Carlini-Wagner (CarliniWagner, input_grad_margin) is not implemented on an EOTTarget: the expectation over "
                                  "transformation is built for the cross-entropy gradient attacks (Attack, L2Attack, APGDAttack)")
