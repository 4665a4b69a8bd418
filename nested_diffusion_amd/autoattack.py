"""AutoAttack's APGD-CE (Linf) on the GPU: a drop-in for the `AutoAttack(model, eps=eps, version='custom', norm='Linf',
attacks_to_run=['apgd-ce'])` the reference builds for --attack_name AUTOPGD (classification_train_separately.py:486, :666) and runs with
`run_standard_evaluation(images, labels, bs=labels.shape[0])` (utils.py:263-266).

autoattack (requirements pin autoattack==0.1, a git install) is not a dependency here, just as foolbox is not: the attack is restated
on the library's kernels (VisionTransformer.input_grad for logits, gradient and per-image cross-entropy; nd_apgd_random_start,
nd_apgd_control, nd_apgd_update for the rest).  Parity is unpinned.  What is restated, from autoattack's published autopgd_base.py /
autoattack.py (all arrays per image; every operation one rounded fp32 op in this order):

    AutoAttack(model, norm='Linf', eps=.3, seed=None, verbose=True, attacks_to_run=[], version='standard', device='cuda')
        apgd = APGDAttack(model, n_restarts=5, n_iter=100, eps=eps, norm=norm, eot_iter=1, rho=.75, seed=seed)
        n_iter_2 = max(int(0.22 n_iter), 1), n_iter_min = max(int(0.06 n_iter), 1), size_decr = max(int(0.03 n_iter), 1)
    run_standard_evaluation(x, y, bs):  robust = argmax(model(x)) == y; for the robust rows, in chunks of bs: adv = apgd.perturb(x, y);
        the rows argmax(model(adv)) misclassifies replace their rows of the output; every other row comes back unchanged
    perturb(x, y):  acc = argmax(model(x)) == y, adv = x; for r < n_restarts: run attack_single_run on the rows with acc still set;
        where it succeeded, acc = 0 and adv = x_best_adv
    attack_single_run(x, y):
        t = 2 U[0,1) - 1;  x_adv = clamp(x + eps * t / (max|t|_image + 1e-12), 0, 1)
        logits, grad, loss = input_grad(x_adv);  acc = argmax(logits) == y;  loss_best = loss;  x_best = x_best_adv = x_adv
        grad_best = grad;  step = 2 eps;  x_adv_old = x_adv;  k = n_iter_2;  counter3 = 0;  loss_best_last_check = loss_best
        reduced_last_check = 1;  loss_steps = zeros[n_iter, B]
        for i < n_iter:
            grad2 = x_adv - x_adv_old;  x_adv_old = x_adv;  a = 1 if i == 0 else 0.75
            z = clamp(min(max(x_adv + step sign(grad), x - eps), x + eps), 0, 1)
            x_adv = clamp(min(max(x_adv + (z - x_adv) a + grad2 (1 - a), x - eps), x + eps), 0, 1)
            logits, grad, loss = input_grad(x_adv)
            pred = argmax(logits) == y;  acc &= pred;  x_best_adv[!pred] = x_adv[!pred]
            loss_steps[i] = loss;  imp = loss > loss_best;  x_best[imp], grad_best[imp], loss_best[imp] = x_adv, grad, loss
            counter3 += 1
            if counter3 == k:
                cnt = #{c < k : loss_steps[i-c] > loss_steps[i-c-1]}          (row -1 is row n_iter-1, as torch indexes)
                osc = cnt <= k rho  or  (reduced_last_check == 0 and loss_best_last_check >= loss_best)
                reduced_last_check = osc;  loss_best_last_check = loss_best
                where osc: step /= 2;  x_adv = x_best;  grad = grad_best
                k = max(k - size_decr, n_iter_min);  counter3 = 0
        return acc, x_best_adv

Deviations, documented: sign(NaN) = 0 (a NaN gradient makes no step); argmax ties go to the first maximal index, and inside
attack_single_run (nd_apgd_control) a NaN logit never wins in any column and a row of NaN logits alone yields index 0, whereas the rows
run_standard_evaluation and perturb select on the host use torch.argmax, where a NaN logit wins: the two differ only for a model
that returns NaN logits, whose row the host then counts as predicting the NaN's class; the random start
draws from the library's Philox keyed on (seed, the image's global index, element, restart) -- the same image starts from the same
point in any batch, subset or rank -- where the reference draws from torch.rand seeded with time.time(); seed=None becomes 0.

The checkpoint schedule is fixed, so the host computes it once; every decision runs on the GPU and an iteration of a restart reads
nothing back to the host (three launches after the input gradient: control, update with the next step fused in).

APGDAttack(norm='L2') is autoattack's APGD-CE in the L2 threat model (AutoAttack(norm='L2')'s first attack), restated from the same
autopgd_base.py; it is reached through APGDAttack directly, which stands on its own like square.SquareAttack (attack_type 'APGD',
epsilon, generate_attack) -- the AutoAttack wrapper stays Linf.  Everything of attack_single_run above is shared (input_grad, the
bookkeeping of nd_apgd_control with step = 2 eps, the checkpoint schedule, x_best / grad_best / x_best_adv, the restore); only the start
and the step differ.  With n(v) = sqrt(sum v^2) per image (the deterministic row reduction of csrc/nd_attack_l2.hip):

        t = N(0, 1);  x_adv = clamp(x + eps * t / (n(t) + 1e-12), 0, 1)
        for i < n_iter:
            grad2 = x_adv - x_adv_old;  x_adv_old = x_adv;  a = 1 if i == 0 else 0.75
            u  = x_adv + step * grad / (n(grad) + 1e-12)
            z  = clamp(x + (u - x) / (n(u - x) + 1e-12) * min(eps, n(u - x)), 0, 1)
            v  = x_adv + (z - x_adv) a + grad2 (1 - a)
            x_adv = clamp(x + (v - x) / (n(v - x) + 1e-12) * min(eps, n(v - x)), 0, 1)

(nd_apgd_l2_random_start, nd_apgd_l2_step; the flags' copies and the restore run before the step, in nd_apgd_update without a step:
six launches after the input gradient).  Deviations, documented: a row whose gradient norm is NaN or infinite takes no gradient step
(u = x_adv), the convention of nd_l2_step; the normals come from the library's Philox and its Box-Muller, keyed as the Linf start is.
Parity is unpinned, as for Linf.

Expectation over transformation (autoattack's eot_iter, AutoAttack version='rand') is not an argument here: eot.EOTTarget wraps the
model instead and composes with every gradient attack.  On this project's two-class datasets DLR and the targeted attacks are
undefined, so APGD-CE on an EOTTarget is what version='rand' reduces to.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Tuple

import torch

from . import ops
from .attack import _vit

# what autoattack's AutoAttack runs for the versions other than 'custom' (set_version), and the attacks it knows
VERSION_ATTACKS = {"standard": ["apgd-ce", "apgd-t", "fab-t", "square"], "plus": ["apgd-ce", "apgd-dlr", "fab", "square", "apgd-t", "fab-t"],
                   "rand": ["apgd-ce", "apgd-dlr"]}
IMPLEMENTED = ("apgd-ce",)
NOT_IMPLEMENTED = ("apgd-t", "apgd-dlr", "fab", "fab-t", "square")


def apgd_schedule(n_iter: int, n_iter_2: int, n_iter_min: int, size_decr: int) -> Dict[int, int]:
    """{iteration i: checkpoint length k} of attack_single_run's step-size checks (counter3 == k)."""
    out, k, counter3 = {}, n_iter_2, 0
    for i in range(n_iter):
        counter3 += 1
        if counter3 == k:
            out[i] = k
            k, counter3 = max(k - size_decr, n_iter_min), 0
    return out


class APGDAttack:
    """autoattack's APGDAttack (autopgd_base.py), norm 'Linf' or 'L2' and the cross-entropy loss: perturb(x, y) -> the adversarial
    batch, and the surface of the other attacks here (attack_type, epsilon, generate_attack) so that attack.apply_attack,
    Diffusion.test_atk(attack=...) and make_attacks.write_attacked_set take it.  `index` (perturb / attack_single_run): the global image
    index of each row, which keys its random start."""

    attack_type = "APGD"

    def __init__(self, predict, n_iter=100, norm="Linf", n_restarts=1, eps=None, seed=0, loss="ce", eot_iter=1, rho=.75, topk=None,
                 verbose=False, device=None, use_largereps=False, is_tf_model=False):
        if norm not in ("Linf", "L2"):
            raise NotImplementedError(f"APGD norm '{norm}' is not implemented (only Linf and L2)")
        if loss != "ce":
            raise NotImplementedError(f"APGD loss '{loss}' is not implemented (only 'ce': apgd-ce)")
        if eot_iter != 1 or use_largereps or is_tf_model:
            raise NotImplementedError("APGD with eot_iter != 1, use_largereps or a TF model is not implemented (for an expectation over "
                                      "transformation wrap the model in eot.EOTTarget)")
        if eps is None:
            raise ValueError("eps is required")
        self.model = _vit(predict)
        self.n_iter, self.norm, self.n_restarts, self.eps = int(n_iter), norm, int(n_restarts), float(eps)
        self.seed = 0 if seed is None else int(seed)
        self.loss, self.eot_iter, self.thr_decr, self.topk, self.verbose = loss, eot_iter, float(rho), topk, verbose
        self.device = device
        self.n_iter_2 = max(int(0.22 * self.n_iter), 1)
        self.n_iter_min = max(int(0.06 * self.n_iter), 1)
        self.size_decr = max(int(0.03 * self.n_iter), 1)
        self.schedule = apgd_schedule(self.n_iter, self.n_iter_2, self.n_iter_min, self.size_decr)

    def attack_single_run(self, x: torch.Tensor, y: torch.Tensor, index: torch.Tensor, restart: int = 0,
                          trace: Optional[Callable] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(acc, x_best_adv) of one run from a random start.  trace(i, logits, grad, loss, arrays, state), if given, is called after
        the start (i = -1) and after each iteration's update; arrays = dict of x_adv, x_adv_old, x_best, grad_best, x_best_adv (x_adv
        already holds the next iterate, except after the last iteration) and state = the ops.ApgdState.  With norm='L2' arrays also
        carries norms [3, B], the per-image norms of the step just taken (nd_apgd_l2_step)."""
        if self.norm == "L2":
            return self._single_run_l2(x, y, index, restart, trace)
        vit, eps = self.model, self.eps
        B = x.shape[0]
        x_adv = ops.apgd_random_start(x, index, eps, self.seed, restart)
        logits, grad, loss = vit.input_grad(x_adv, y)
        st = ops.ApgdState(B, self.n_iter, x.device)
        ops.apgd_control(logits, y, loss, st, -1, 0, self.thr_decr, step0=2.0 * eps)
        x_best, x_best_adv, grad_best, x_adv_old = x_adv.clone(), x_adv.clone(), grad.clone(), x_adv.clone()
        arrays = dict(x_adv=x_adv, x_adv_old=x_adv_old, x_best=x_best, grad_best=grad_best, x_best_adv=x_best_adv)
        if trace is not None:
            trace(-1, logits, grad, loss, arrays, st)
        ops.apgd_update(x, x_adv, x_adv_old, grad, None, None, None, None, st.step, eps, 1.0, True)      # the first step: a = 1
        for i in range(self.n_iter):
            logits, grad, loss = vit.input_grad(x_adv, y)
            flags = ops.apgd_control(logits, y, loss, st, i, self.schedule.get(i, 0), self.thr_decr)
            ops.apgd_update(x, x_adv, x_adv_old, grad, x_best, grad_best, x_best_adv, flags, st.step, eps, 0.75, i + 1 < self.n_iter)
            if trace is not None:
                trace(i, logits, grad, loss, arrays, st)
        return st.acc.bool(), x_best_adv

    def _single_run_l2(self, x, y, index, restart, trace):
        """attack_single_run with the L2 start and step: the update without a step makes the flags' copies and the restore, then
        nd_apgd_l2_step moves x_adv."""
        vit, eps = self.model, self.eps
        B = x.shape[0]
        x_adv = ops.apgd_l2_random_start(x, index, eps, self.seed, restart)
        logits, grad, loss = vit.input_grad(x_adv, y)
        st = ops.ApgdState(B, self.n_iter, x.device)
        ops.apgd_control(logits, y, loss, st, -1, 0, self.thr_decr, step0=2.0 * eps)
        x_best, x_best_adv, grad_best, x_adv_old = x_adv.clone(), x_adv.clone(), grad.clone(), x_adv.clone()
        arrays = dict(x_adv=x_adv, x_adv_old=x_adv_old, x_best=x_best, grad_best=grad_best, x_best_adv=x_best_adv)
        if trace is not None:
            trace(-1, logits, grad, loss, arrays, st)
        arrays["norms"] = ops.apgd_l2_step(x, x_adv, x_adv_old, grad, None, None, st.step, eps, 1.0)    # the first step: a = 1
        for i in range(self.n_iter):
            logits, grad, loss = vit.input_grad(x_adv, y)
            flags = ops.apgd_control(logits, y, loss, st, i, self.schedule.get(i, 0), self.thr_decr)
            ops.apgd_update(None, x_adv, None, grad, x_best, grad_best, x_best_adv, flags, None, eps, 0.75, False)
            if i + 1 < self.n_iter:
                arrays["norms"] = ops.apgd_l2_step(x, x_adv, x_adv_old, grad, grad_best, flags, st.step, eps, 0.75)
            if trace is not None:
                trace(i, logits, grad, loss, arrays, st)
        return st.acc.bool(), x_best_adv

    @property
    def epsilon(self) -> float:
        """eps under the name the other attacks (and write_attacked_set) use."""
        return self.eps

    def generate_attack(self, samples: torch.Tensor, labels: torch.Tensor, first_image: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
        """(adversarial images, success), as the other attacks: rows the clean model misclassifies and rows no restart fools come back
        unchanged; first_image is the global index of samples[0]."""
        dev = self.model.device
        labels = labels.to(dev, torch.int64).contiguous()
        adv = self.perturb(samples, labels, index=first_image + torch.arange(samples.shape[0], dtype=torch.int64))
        success = self.model.forward(adv).argmax(dim=1) != labels if adv.shape[0] else torch.zeros(0, dtype=torch.bool, device=adv.device)
        return adv, success

    def perturb(self, x: torch.Tensor, y: torch.Tensor, index: Optional[torch.Tensor] = None) -> torch.Tensor:
        dev = self.model.device
        x = x.to(dev, torch.float32).contiguous()
        y = y.to(dev, torch.int64).contiguous()
        index = (torch.arange(x.shape[0]) if index is None else index).to(dev, torch.int64)
        acc = self.model.forward(x).argmax(dim=1) == y
        adv = x.clone()
        for r in range(self.n_restarts):
            ind = acc.nonzero().flatten()
            if ind.numel() == 0:
                break
            acc_curr, adv_curr = self.attack_single_run(x[ind].contiguous(), y[ind].contiguous(), index[ind].contiguous(), restart=r)
            succ = ~acc_curr
            acc[ind[succ]] = False
            adv[ind[succ]] = adv_curr[succ]
        return adv


class AutoAttack:
    """autoattack's AutoAttack restricted to what the reference runs: norm='Linf', version='custom', attacks_to_run ⊆ ['apgd-ce'].
    attack_type = "AUTOPGD": runner.test_atk(attack=...) hands it to attack.apply_attack, which calls run_standard_evaluation."""

    attack_type = "AUTOPGD"

    def __init__(self, model, norm="Linf", eps=.3, seed=None, verbose=True, attacks_to_run=[], version="standard", device="cuda"):
        if norm != "Linf":
            raise NotImplementedError(f"AutoAttack norm '{norm}' is not implemented (only Linf)")
        if version != "custom":
            runs = VERSION_ATTACKS.get(version)
            what = f" (it runs {', '.join(runs)})" if runs else ""
            raise NotImplementedError(f"AutoAttack version '{version}' is not implemented{what}: only version='custom' with "
                                      f"attacks_to_run=['apgd-ce']")
        bad = [a for a in attacks_to_run if a not in IMPLEMENTED]
        if bad:
            raise NotImplementedError(f"AutoAttack attacks {', '.join(repr(a) for a in bad)} are not implemented (only 'apgd-ce'; "
                                      "Square stands on its own as square.SquareAttack)")
        self.model = _vit(model)
        self.norm, self.epsilon, self.seed, self.verbose = norm, float(eps), seed, verbose
        self.attacks_to_run: List[str] = list(attacks_to_run)
        self.version, self.device = version, device
        self.apgd = APGDAttack(self.model, n_restarts=5, n_iter=100, eps=self.epsilon, norm=norm, eot_iter=1, rho=.75, seed=seed,
                               device=device)

    def get_seed(self) -> int:
        return 0 if self.seed is None else int(self.seed)

    def run_standard_evaluation(self, x_orig: torch.Tensor, y_orig: torch.Tensor, bs: int = 250, first_image: int = 0) -> torch.Tensor:
        """The adversarial batch: rows the clean model already misclassifies and rows no restart fools come back unchanged.
        first_image: the global index of x_orig[0] (its index in the dataset or test stream), which keys each image's random start."""
        dev = self.model.device
        x = x_orig.to(dev, torch.float32).contiguous()
        y = y_orig.to(dev, torch.int64).contiguous()
        n = x.shape[0]
        bs = max(int(bs), 1)
        robust = torch.cat([self.model.forward(x[s:s + bs]).argmax(dim=1) == y[s:s + bs] for s in range(0, n, bs)]) if n else \
            torch.zeros(0, dtype=torch.bool, device=dev)
        x_adv = x.clone()
        for attack in self.attacks_to_run:                # only 'apgd-ce' gets here
            ids = robust.nonzero().flatten()
            if ids.numel() == 0:
                break
            self.apgd.seed = self.get_seed()
            for s in range(0, ids.numel(), bs):
                b = ids[s:s + bs]
                xb, yb = x[b].contiguous(), y[b].contiguous()
                adv_curr = self.apgd.perturb(xb, yb, index=first_image + b)
                false = self.model.forward(adv_curr).argmax(dim=1) != yb
                robust[b[false]] = False
                x_adv[b[false]] = adv_curr[false]
        return x_adv


class WorstCase:
    """AutoAttack's evaluation order for any list of attacks that have perturb(x, y, index=), norm and eps: the per-image worst case.
    Rows the clean model gets wrong come back unchanged; each attack, in the order given, sees only the rows still robust, with their
    global indices; the first adversarial found for a row is kept, and robust_after records (name, robust count) after each attack.
    On this project's two-class datasets the L2 evaluation is WorstCase(t, [APGDAttack(t, norm='L2', ...), SquareL2Attack(t, ...)]):
    APGD-T, APGD-DLR and FAB-T are undefined with two classes.  attack_type = "WORSTCASE", epsilon and generate_attack: the surface
    attack.apply_attack, Diffusion.test_atk(attack=...) and make_attacks.write_attacked_set take."""

    attack_type = "WORSTCASE"

    def __init__(self, model, attacks):
        attacks = list(attacks)
        if not attacks:
            raise ValueError("WorstCase needs at least one attack")
        for a in attacks:
            if not callable(getattr(a, "perturb", None)) or not hasattr(a, "norm") or not hasattr(a, "eps"):
                raise TypeError(f"WorstCase members need perturb(x, y, index=), norm and eps ({self._name(a)} does not)")
        first = attacks[0]
        for a in attacks[1:]:
            if a.norm != first.norm or float(a.eps) != float(first.eps):
                raise ValueError(f"WorstCase members disagree on the threat model: {self._name(first)} has norm={first.norm!r}, eps={first.eps!r} "
                                 f"and {self._name(a)} has norm={a.norm!r}, eps={a.eps!r}")
        self.model = _vit(model)
        forward = getattr(self.model, "forward", self.model)
        if not callable(forward):
            raise TypeError("model must have forward(x) -> [B, C] scores or be such a callable")
        self.predict = forward
        self.attacks = attacks
        self.norm, self.eps = first.norm, float(first.eps)
        self.epsilon = self.eps
        self.robust_after: List[Tuple[str, int]] = []

    @staticmethod
    def _name(a) -> str:
        return str(getattr(a, "attack_type", type(a).__name__))

    def perturb(self, x: torch.Tensor, y: torch.Tensor, index: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The adversarial batch; fills robust_after with ("clean", n) and one entry per attack that ran."""
        dev = getattr(self.model, "device", None) or x.device
        x = x.to(dev, torch.float32).contiguous()
        y = y.to(dev, torch.int64).contiguous()
        index = (torch.arange(x.shape[0]) if index is None else index).to(dev, torch.int64)
        adv = x.clone()
        robust = self.predict(x).argmax(dim=1) == y if x.shape[0] else torch.zeros(0, dtype=torch.bool, device=dev)
        self.robust_after = [("clean", int(robust.sum()))]
        for a in self.attacks:
            ids = robust.nonzero().flatten()
            if ids.numel() == 0:
                break
            xb, yb = x[ids].contiguous(), y[ids].contiguous()
            adv_curr = a.perturb(xb, yb, index=index[ids].contiguous()).to(dev)
            fooled = self.predict(adv_curr).argmax(dim=1) != yb
            robust[ids[fooled]] = False
            adv[ids[fooled]] = adv_curr[fooled]
            self.robust_after.append((self._name(a), int(robust.sum())))
        return adv

    def generate_attack(self, samples: torch.Tensor, labels: torch.Tensor, first_image: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
        """(adversarial images, success), as the other attacks; first_image is the global index of samples[0]."""
        adv = self.perturb(samples, labels, index=first_image + torch.arange(samples.shape[0], dtype=torch.int64))
        labels = labels.to(adv.device, torch.int64)
        success = self.predict(adv).argmax(dim=1) != labels if adv.shape[0] else torch.zeros(0, dtype=torch.bool, device=adv.device)
        return adv, success
