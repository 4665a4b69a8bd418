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

The L2 family (L2Attack: 'BIM' = L2BasicIterativeAttack, 'L2PGD' = L2ProjectedGradientDescentAttack) restates foolbox 3.x's
L2BaseGradientDescent on nd_l2_step / nd_l2_random_start (parity unpinned, as above); all norms are per image:

    x = clip(x0 + eps * r, 0, 1) if random_start else x0
          # r: uniform in the unit n-ball, n = 3*H*W
    repeat steps:
        g = d/dx crossentropy(model(x), labels).sum()
        x = x + stepsize * (g * (1 / max(||g||_2, 1e-12)))
        d = x - x0
        x = x0 + d * min(1, eps / max(||d||_2, 1e-12))
        x = clip(x, 0, 1)
    adv = x0 + p * min(1, eps / max(||p||_2, 1e-12)),  p = x - x0
          # the final clip_perturbation
    success = argmax(model(adv)) != labels

r follows foolbox's uniform_n_balls: n + 2 standard normals per image, divided by their L2 norm over all n + 2, the first n kept.  The
normals come from the library's Philox generator keyed on (seed, the image's global index, element, restart).

Carlini & Wagner's L2 attack (CarliniWagner) restates foolbox 3.x's L2CarliniWagnerAttack (parity unpinned) on nd_cw_attack_space,
nd_cw_model_space, VisionTransformer.input_grad_margin, nd_cw_control and nd_cw_update; a = 0.5, b = 0.5 for bounds (0, 1):

    w0   = atanh(((x0 - a) / b) * 0.999999)
    xrec = tanh(w0) * b + a
    consts = initial_const        (float64 on the host, one per image)
    lower = 0;  upper = inf
    best = zeros_like(x0);  best_norm = inf
    for bs in range(binary_search_steps):
        if bs == binary_search_steps - 1 and binary_search_steps >= 10:
            consts = min(upper, 1e10)
        delta = 0;  Adam state m = v = 0;  found = False;  prev = inf
        c = float32(consts)
        for k in range(steps):
            t = tanh(w0 + delta);  x = t * b + a;  logits = model(x)
            other  = first maximal index of logits with the label's column excluded
            margin = logits[label] - logits[other] + confidence
            loss_b = c_b * max(0, margin_b) + sum((x_b - xrec_b)^2)
            g = d(sum_b loss_b) / d(delta)
              = (dx + 2 (x - xrec)) * b * (1 - t^2)
                # dx = d/dx sum_b c_b max(0, margin_b)
            m = 0.9 m + 0.1 g;  v = 0.999 v + 0.001 g^2
            delta -= stepsize * (m / (1 - 0.9^(k+1)))
                              / (sqrt(v / (1 - 0.999^(k+1))) + 1e-8)
            if abort_early and k % ceil(steps / 10) == 0:
                if not (sum_b loss_b <= 0.9999 * prev): break
                prev = sum_b loss_b
            adv_b   = argmax(logits_b + confidence * onehot(label_b)) != label_b
            found  |= adv
            norm_b  = ||x_b - x0_b||_2
            new_best = adv & (norm < best_norm)
            best[new_best] = x[new_best]
            best_norm[new_best] = norm[new_best]
        upper = where(found, consts, upper)
        lower = where(found, lower, consts)
        consts = where(isinf(upper), consts * 10, (lower + upper) / 2)
    adv = x0 + p * min(1, eps / max(||p||_2, 1e-12)),  p = best - x0
    success = argmax(model(adv)) != labels

The bookkeeping of an iteration uses x and logits from before that iteration's Adam update.  An image that never becomes adversarial
keeps best = 0 and returns the clipped step from x0 towards the zero image: that is foolbox's behaviour, kept here.  The abort-early read
comes before the iteration's Adam update is queued: the update of an aborting iteration would go into a delta that is discarded, and its
bookkeeping is skipped, as in the listing.  The only host synchronisation inside a binary-search step is that read of the B per-image
losses every ceil(steps / 10) iterations; the constants are updated on the host in float64 once per binary-search step.
"""
from __future__ import annotations

import math
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
# attack_type -> (foolbox class, rel_stepsize, steps, random_start) of the L2 family (L2Attack): foolbox 3.x defaults (unpinned)
L2_ATTACKS = {
    "BIM": ("L2BasicIterativeAttack", 0.2, 10, False),
    "L2PGD": ("L2ProjectedGradientDescentAttack", 0.025, 50, True),
}
# names class Attack refuses: the L2 family (L2Attack) and Carlini & Wagner (CarliniWagner) stand beside it and make_attack picks among
# them; AutoAttack's APGD, which the reference's Attack class has no branch for either, is autoattack.AutoAttack (apply_attack's 'AUTOPGD')
NOT_IMPLEMENTED = ("CW", "BIM", "L2PGD", "AUTOPGD")


def _vit(model):
    """The model the reference attacks is cond_pred_model['vit']; a GuidingConditioner is accepted for its ViT."""
    return getattr(model, "vit", model)


class _GradientDescentAttack:
    """What foolbox's Linf and L2 gradient-descent attacks share (the loops are in the module docstring): a subclass names its table
    (attack_type -> (foolbox class, rel_stepsize, steps, random_start)) and the two ops calls that differ, _random_start and _step."""

    TABLE: dict = {}
    _random_start = _step = None                 # staticmethod(ops.<norm>_random_start), staticmethod(ops.<norm>_step)

    def __init__(self, epsilon: float, attack_type: str, model, seed: int = 0):
        self._check_type(attack_type)
        self.epsilon, self.attack_type, self.model, self.seed = float(epsilon), attack_type, _vit(model), int(seed)
        _, self.rel_stepsize, self.steps, self.random_start = self.TABLE[attack_type]
        self.stepsize = self.rel_stepsize * self.epsilon

    def start(self, x0: torch.Tensor, first_image: int = 0) -> torch.Tensor:
        """The first iterate: x0, or (random_start) the family's random point of the eps-ball around x0, clipped to (0, 1)."""
        if not self.random_start:
            return x0
        return self._random_start(x0, self.epsilon, self.seed, first_image, 0, *BOUNDS)

    def step(self, x: torch.Tensor, x0: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        """One gradient step from x (gradient on the GPU, then the family's step, projection onto the eps-ball, clip)."""
        _, g, _ = self.model.input_grad(x, labels)
        return self._step(x, x0, g, self.stepsize, self.epsilon, *BOUNDS)

    def generate_attack(self, samples: torch.Tensor, labels: torch.Tensor, first_image: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
        dev = self.model.device
        x0 = samples.to(dev, torch.float32).contiguous()
        labels = labels.to(dev, torch.int64).contiguous()
        x = self.start(x0, first_image)
        for _ in range(self.steps):
            x = self.step(x, x0, labels)
        adv = self._step(x, x0, None, 0.0, self.epsilon, float("-inf"), float("inf"))       # clip_perturbation
        success = self.model.forward(adv).argmax(dim=1) != labels
        return adv, success


class Attack(_GradientDescentAttack):
    """attack.py's Attack(epsilon, attack_type, model): generate_attack(samples, labels) -> (adversarial images, success).
    seed: key of the PGD random start (clip(x0 + U[-eps, eps), 0, 1)).  first_image (generate_attack): the global index of samples[0]
    (its index in the dataset or test stream), which keys each image's random start."""

    TABLE = LINF_ATTACKS
    _random_start, _step = staticmethod(ops.linf_random_start), staticmethod(ops.linf_step)

    @staticmethod
    def _check_type(attack_type: str) -> None:
        if attack_type in NOT_IMPLEMENTED:
            raise NotImplementedError(f"attack '{attack_type}' is not implemented by class Attack (only the Linf family: {', '.join(LINF_ATTACKS)}; "
                                      "see make_attack, L2Attack, CarliniWagner, autoattack.AutoAttack)")
        if attack_type not in LINF_ATTACKS:
            raise ValueError(f"Attacks of type {attack_type} is not supported")


class L2Attack(_GradientDescentAttack):
    """foolbox's L2 gradient-descent attacks ('BIM', 'L2PGD') with the surface of Attack: generate_attack(samples, labels) ->
    (adversarial images, success); the loop is in the module docstring.  seed keys the random start of L2PGD (clip(x0 + eps * r, 0, 1), r
    uniform in the unit ball), first_image is the global index of samples[0]."""

    TABLE = L2_ATTACKS
    _random_start, _step = staticmethod(ops.l2_random_start), staticmethod(ops.l2_step)

    @staticmethod
    def _check_type(attack_type: str) -> None:
        if attack_type not in L2_ATTACKS:
            raise ValueError(f"Attacks of type {attack_type} is not supported (the L2 family: {', '.join(L2_ATTACKS)})")


class CarliniWagner:
    """foolbox's L2CarliniWagnerAttack(binary_search_steps, steps, stepsize, confidence) as the reference's CW branch calls it
    (6, 1000, 0.01, 0): generate_attack(samples, labels) -> (adversarial images, success); the loop is in the module docstring.
    An image that never becomes adversarial returns the clipped step from x0 towards the zero image (foolbox's behaviour)."""

    attack_type = "CW"

    def __init__(self, epsilon: float, model, binary_search_steps: int = 6, steps: int = 1000, stepsize: float = 0.01,
                 confidence: float = 0.0, initial_const: float = 1e-3, abort_early: bool = True):
        if binary_search_steps < 1 or steps < 1:
            raise ValueError("binary_search_steps and steps must be at least 1")
        self.epsilon, self.model = float(epsilon), _vit(model)
        from .ensemble_grad import EnsembleTarget
        from .mapping import ConditionerTarget
        if isinstance(self.model, (ConditionerTarget, EnsembleTarget)):   # refused here, by name, not by an AttributeError in the first iteration
            self.model.input_grad_margin()
        self.binary_search_steps, self.steps, self.stepsize = int(binary_search_steps), int(steps), float(stepsize)
        self.confidence, self.initial_const, self.abort_early = float(confidence), float(initial_const), bool(abort_early)

    @staticmethod
    def _read_losses(loss: torch.Tensor) -> float:
        """The abort-early read: the B per-image losses of an iteration, summed in float64 (the loop's only host synchronisation)."""
        return float(loss.double().sum())

    def generate_attack(self, samples: torch.Tensor, labels: torch.Tensor, first_image: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
        """first_image is accepted for apply_attack's signature and unused: CW draws nothing."""
        dev = self.model.device
        x0 = samples.to(dev, torch.float32).contiguous()
        labels = labels.to(dev, torch.int64).contiguous()
        B = x0.shape[0]
        n_cls = self.model.p["head.weight"].shape[0]
        if B and (int(labels.min()) < 0 or int(labels.max()) >= n_cls):      # once, so that the iterations need not read the labels back
            raise ValueError(f"labels must lie in [0, {n_cls})")
        w0, xrec = ops.cw_attack_space(x0, *BOUNDS)
        s = ops.CwState(x0)
        consts = torch.full((B,), self.initial_const, dtype=torch.float64)
        lower, upper = torch.zeros(B, dtype=torch.float64), torch.full((B,), float("inf"), dtype=torch.float64)
        every = math.ceil(self.steps / 10)
        for bs in range(self.binary_search_steps):
            if bs == self.binary_search_steps - 1 and self.binary_search_steps >= 10:
                consts = torch.minimum(upper, torch.full_like(upper, 1e10))
            s.reset_search_step()
            c = consts.to(torch.float32).to(dev)
            prev = float("inf")
            for k in range(self.steps):
                x = ops.cw_model_space(w0, x0, xrec, s, *BOUNDS)
                logits, dx, margin = self.model.input_grad_margin(x, labels, c, self.confidence, check_labels=False)
                if self.abort_early and k % every == 0:
                    # read before nd_cw_control runs: an aborting iteration leaves found and best alone
                    total = self._read_losses(self._loss(c, margin, s.sq_rec))
                    if not total <= 0.9999 * prev:
                        break
                    prev = total
                ops.cw_control(logits, labels, c, margin, s, self.confidence)
                ops.cw_update(s, dx, xrec, self.stepsize, k, *BOUNDS)
            found = s.found.cpu().bool()
            upper = torch.where(found, consts, upper)
            lower = torch.where(found, lower, consts)
            consts = torch.where(torch.isinf(upper), consts * 10, (lower + upper) / 2)
        self.last_best_norm = s.best_norm                    # per image, over all binary-search steps: inf where nothing was found
        adv = ops.l2_step(s.best, x0, None, 0.0, self.epsilon, float("-inf"), float("inf"))  # clip_perturbation
        success = self.model.forward(adv).argmax(dim=1) != labels
        return adv, success

    @staticmethod
    def _loss(c: torch.Tensor, margin: torch.Tensor, sq_rec: torch.Tensor) -> torch.Tensor:
        """loss_b = c_b * max(0, margin_b) + sq_rec_b on B scalars: nd_cw_control's expression, needed before it runs on a check iteration."""
        return c * torch.where(margin > 0, margin, torch.zeros_like(margin)) + sq_rec


def make_attack(epsilon: float, attack_type: str, model, seed: int = 0):
    """All six names of the reference's Attack class: an Attack (FGSM, PGD, LinfBIM), an L2Attack (BIM, L2PGD) or a CarliniWagner (CW)
    with the reference's arguments (6, 1000, 0.01, 0)."""
    if attack_type in LINF_ATTACKS:
        return Attack(epsilon, attack_type, model, seed=seed)
    if attack_type in L2_ATTACKS:
        return L2Attack(epsilon, attack_type, model, seed=seed)
    if attack_type == "CW":
        return CarliniWagner(epsilon, model, binary_search_steps=6, steps=1000, stepsize=0.01, confidence=0.0)
    raise ValueError(f"Attacks of type {attack_type} is not supported")


def apply_attack(attack_func, images_in: torch.Tensor, labels_in: torch.Tensor, attack_name: str,
                 first_image: int = 0) -> torch.Tensor:
    """utils.py:258-269: the adversarial images of a batch (the inputs are not modified).  attack_func is anything with
    generate_attack(samples, labels, first_image=) -- an Attack, an L2Attack, a CarliniWagner, a square.SquareAttack or SquareL2Attack, an
    autoattack.APGDAttack or an autoattack.WorstCase; AUTOPGD takes an autoattack.AutoAttack
    (run_standard_evaluation with bs = the batch, as utils.py:263-266 calls it)."""
    if attack_name == "AUTOPGD":
        from .autoattack import AutoAttack
        if not isinstance(attack_func, AutoAttack):
            raise NotImplementedError("attack 'AUTOPGD' needs an autoattack.AutoAttack (AutoAttack's run_standard_evaluation)")
        return attack_func.run_standard_evaluation(images_in.clone(), labels_in.clone(), bs=labels_in.shape[0], first_image=first_image)
    adv, _ = attack_func.generate_attack(images_in.clone(), labels_in.clone(), first_image=first_image)
    return adv

