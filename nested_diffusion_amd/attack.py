"""Adversarial examples on the GPU: a drop-in for the reference's attack.py (class Attack) and utils.apply_attack (utils.py:258-269).

The reference wraps cond_pred_model['vit'] -- the full timm ViT-B/16 -- in foolbox 3.x (fb.models.PyTorchModel(model, bounds=(0, 1)))
and calls its attacks with one scalar epsilon.  foolbox is not a dependency here: the Linf family is restated on the library's own
kernels (VisionTransformer.input_grad for the gradient, nd_linf_step / nd_linf_random_start for the steps).  The constants and the loop
below restate foolbox 3.x's LinfBaseGradientDescent (unpinned: the reference's requirements do not pin foolbox):

    x0 = inputs
    x = clip(x0 + U[-eps, eps), *bounds) if random_start else x0
    repeat steps times:  g = d/dx crossentropy(model(x), labels).sum()
                         x = clip(x0 + clip(x + stepsize * sign(g) - x0, -eps, eps), *bounds)
    adv = x0 + clip(x - x0, -eps, eps)                   (the attack's final clip_perturbation)
    success = argmax(model(adv)) != labels              (Misclassification)

with stepsize = rel_stepsize * eps.  The random start draws from the library's counter-based Philox generator keyed on (seed, the
image's global index, element, restart): the same image starts from the same point at any batch size and on any rank (foolbox draws
from the torch generator, which no GPU run can reproduce).
"""
from __future__ import annotations

from typing import Tuple

import torch

from . import ops

BOUNDS = (0.0, 1.0)                          # fb.models.PyTorchModel(model, bounds=(0, 1)), attack.py

# attack_type -> (foolbox class, rel_stepsize, steps, random_start): foolbox 3.x defaults (unpinned)
LINF_ATTACKS = {
    "FGSM": ("LinfFastGradientAttack", 1.0, 1, False),
    "PGD": ("LinfProjectedGradientDescentAttack", 0.01 / 0.3, 40, True),
    "LinfBIM": ("LinfBasicIterativeAttack", 0.2, 10, False),
}
# the reference's other attacks: the L2 family, Carlini & Wagner, and AutoAttack's APGD, which its Attack class has no branch for either
# (apply_attack's 'AUTOPGD' branch takes an autoattack.AutoAttack)
NOT_IMPLEMENTED = ("CW", "BIM", "L2PGD", "AUTOPGD")


def _vit(model):
    """The model the reference attacks is cond_pred_model['vit']; a GuidingConditioner is accepted for its ViT."""
    return getattr(model, "vit", model)


class Attack:
    """attack.py's Attack(epsilon, attack_type, model): generate_attack(samples, labels) -> (adversarial images, success).
    seed: key of the PGD random start.  first_image (generate_attack): the global index of samples[0] (its index in the dataset or test
    stream), which keys each image's random start."""

    def __init__(self, epsilon: float, attack_type: str, model, seed: int = 0):
        if attack_type in NOT_IMPLEMENTED:
            raise NotImplementedError(f"attack '{attack_type}' is not implemented (only the Linf family: {', '.join(LINF_ATTACKS)})")
        if attack_type not in LINF_ATTACKS:
            raise ValueError(f"Attacks of type {attack_type} is not supported")
        self.epsilon, self.attack_type, self.model, self.seed = float(epsilon), attack_type, _vit(model), int(seed)
        _, self.rel_stepsize, self.steps, self.random_start = LINF_ATTACKS[attack_type]
        self.stepsize = self.rel_stepsize * self.epsilon

    def start(self, x0: torch.Tensor, first_image: int = 0) -> torch.Tensor:
        """The first iterate: x0, or (random_start) clip(x0 + U[-eps, eps), 0, 1)."""
        if not self.random_start:
            return x0
        return ops.linf_random_start(x0, self.epsilon, self.seed, first_image, 0, *BOUNDS)

    def step(self, x: torch.Tensor, x0: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        """One gradient step from x (gradient on the GPU, then step, project, clip)."""
        _, g, _ = self.model.input_grad(x, labels)
        return ops.linf_step(x, x0, g, self.stepsize, self.epsilon, *BOUNDS)

    def generate_attack(self, samples: torch.Tensor, labels: torch.Tensor, first_image: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
        dev = self.model.device
        x0 = samples.to(dev, torch.float32).contiguous()
        labels = labels.to(dev, torch.int64).contiguous()
        x = self.start(x0, first_image)
        for _ in range(self.steps):
            x = self.step(x, x0, labels)
        adv = ops.linf_step(x, x0, None, 0.0, self.epsilon, float("-inf"), float("inf"))     # clip_perturbation
        success = self.model.forward(adv).argmax(dim=1) != labels
        return adv, success


def apply_attack(attack_func: Attack, images_in: torch.Tensor, labels_in: torch.Tensor, attack_name: str,
                 first_image: int = 0) -> torch.Tensor:
    """utils.py:258-269: the adversarial images of a batch (the inputs are not modified).  AUTOPGD takes an autoattack.AutoAttack
    (run_standard_evaluation with bs = the batch, as utils.py:263-266 calls it)."""
    if attack_name == "AUTOPGD":
        from .autoattack import AutoAttack
        if not isinstance(attack_func, AutoAttack):
            raise NotImplementedError("attack 'AUTOPGD' needs an autoattack.AutoAttack (AutoAttack's run_standard_evaluation)")
        return attack_func.run_standard_evaluation(images_in.clone(), labels_in.clone(), bs=labels_in.shape[0], first_image=first_image)
    adv, _ = attack_func.generate_attack(images_in.clone(), labels_in.clone(), first_image=first_image)
    return adv

