"""Drop-in mirror of the reference's diffusion/diffusion_utils.py for the inference path:
same function names, argument order and return conventions; the arithmetic runs in libnd_hip.so.

Training-only functions of the reference module (q_sample :39-50, y_0_reparam :114-130) are out
of scope.
"""
from __future__ import annotations

import math
from collections import namedtuple
from typing import List, Optional, Sequence, Union

import torch


def _cosine_alpha_bar(u: float, s: float = 0.008) -> float:
    return math.cos((u + s) / (1 + s) * math.pi / 2) ** 2


def make_beta_schedule(schedule="linear", num_timesteps=1000, start=1e-5, end=1e-2):
    """Noise schedule beta_1..beta_T (reference: diffusion_utils.py:5-28; same names, same fp32 torch ops per branch, so
    the tables are bit-identical -- pinned by tests/golden/schedule.npz).  Init-time host table of T floats."""
    T = num_timesteps
    if schedule == "linear":
        return torch.linspace(start, end, T)
    if schedule == "const":
        return end * torch.ones(T)
    if schedule == "quad":
        return torch.linspace(start ** 0.5, end ** 0.5, T) ** 2
    if schedule == "jsd":
        return 1.0 / torch.linspace(T, 1, T)
    if schedule == "sigmoid":
        return torch.sigmoid(torch.linspace(-6, 6, T)) * (end - start) + start
    if schedule in ("cosine", "cosine_reverse"):
        # beta_i = min(1 - abar((i+1)/T) / abar(i/T), 0.999), abar(u) = cos^2(((u + 0.008) / 1.008) * pi / 2)
        return torch.tensor([min(1 - _cosine_alpha_bar((i + 1) / T) / _cosine_alpha_bar(i / T), 0.999) for i in range(T)])
    if schedule == "cosine_anneal":
        return torch.tensor([start + 0.5 * (end - start) * (1 - math.cos(t / (T - 1) * math.pi)) for t in range(T)])
    raise ValueError(f"unknown beta schedule '{schedule}'")


ScheduleTables = namedtuple("ScheduleTables", "betas alphas alphas_bar_sqrt one_minus_alphas_bar_sqrt")


def schedule_tables(schedule, num_timesteps, start, end) -> ScheduleTables:
    """The T-float tables every user of the schedule reads (classification_train_separately.py:215-226): fp32 on the CPU, the reference's
    torch ops in the reference's order (CPU cumprod), so that every caller holds the same bits -- pinned by tests/golden/schedule.npz.
    The cosine schedule's 0.9999 goes on one_minus_alphas_bar_sqrt only, as there.  Callers move the tables where they need them."""
    betas = make_beta_schedule(schedule=schedule, num_timesteps=num_timesteps, start=start, end=end).float()
    alphas = 1.0 - betas
    alphas_cumprod = alphas.cumprod(dim=0)
    one_minus_alphas_bar_sqrt = torch.sqrt(1 - alphas_cumprod)
    if schedule == "cosine":
        one_minus_alphas_bar_sqrt = one_minus_alphas_bar_sqrt * 0.9999
    return ScheduleTables(betas, alphas, torch.sqrt(alphas_cumprod), one_minus_alphas_bar_sqrt)


def extract(input, t, x):
    """diffusion_utils.py:31-35 (table lookup reshaped for broadcasting; host plumbing)."""
    shape = x.shape
    out = torch.gather(input, 0, t.to(input.device))
    reshape = [t.shape[0]] + [1] * (len(shape) - 1)
    return out.reshape(*reshape)


def draw_reference_noise(n_steps: int, like: torch.Tensor, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """The T draws of p_sample_loop in the reference's order (:139 then :67 for t = T-1 .. 1), made on
    the CPU generator exactly as the reference's CPU path makes them: n_steps successive
    randn of like.shape.  With torch.manual_seed(s) before both, the noise is identical to what the
    reference consumes on CPU -- this is how parity runs are driven."""
    shape = tuple(like.shape)
    return torch.stack([torch.randn(shape, generator=generator) for _ in range(n_steps)])


SKIP_TYPES = ("uniform", "quadratic")
SamplerPlan = namedtuple("SamplerPlan", "timesteps coef")


def timestep_sequence(T: int, S: int, skip_type: str = "uniform") -> List[int]:
    """The timesteps tau_0 < .. < tau_{S'-1} of a sampler plan over a schedule of T steps: 'uniform' round(linspace(0, T-1, S)),
    'quadratic' round(linspace(0, sqrt(T-1), S)^2), both formed in double, rounded and de-duplicated, so both start at 0 and end at
    T-1 (S = 1: [0]) and S' <= S (S >= T gives every timestep).  Ours, not the reference's: its --skip_type is declared and never read."""
    T, S = int(T), int(S)
    if T < 1:
        raise ValueError(f"a schedule has at least one timestep (T={T})")
    if S < 1:
        raise ValueError(f"a sampler plan has at least one step (S={S})")
    if skip_type not in SKIP_TYPES:
        raise ValueError(f"skip_type must be one of {SKIP_TYPES}, got {skip_type!r}")
    if S == 1:
        return [0]
    if S >= T:
        return list(range(T))
    import numpy as np
    pts = np.linspace(0.0, T - 1.0, S) if skip_type == "uniform" else np.linspace(0.0, math.sqrt(T - 1.0), S) ** 2     # float64
    seq = {min(T - 1, max(0, int(v))) for v in np.round(pts)}               # numpy rounds halves to even
    return sorted(seq | {0, T - 1})


def sampler_plan(one_minus_alphas_bar_sqrt: torch.Tensor, timesteps: Sequence[int], eta: float = 1.0) -> SamplerPlan:
    """(timesteps [S] int32, coef [S, 4] float32 = (cy, cm, ce, cz)) of the reverse chain over the increasing subsequence `timesteps` of
    the schedule (include/nested_diffusion.h, "SAMPLER PLAN"): with abar_t = 1 - s_t^2 from the fp32 table s, row j >= 1 is the step
    from t = tau_j to r = tau_{j-1},
        sigma = eta sqrt((1 - abar_r) / (1 - abar_t)) sqrt(1 - abar_t / abar_r),  cy = sqrt(abar_r / abar_t),  cm = 1 - cy,
        ce = sqrt(1 - abar_r - sigma^2) - cy sqrt(1 - abar_t),  cz = sigma,
    and row 0 is p_sample_t_1to0 at tau_0: cy = 1 / sqrt(abar), cm = -(1 - sqrt(abar)) / sqrt(abar), ce = -sqrt(1 - abar) / sqrt(abar),
    cz = 0.  Formed in double and rounded once (as ensemble_grad.reverse_step_coefficients).  eta = 1 is the reference's posterior on the
    sub-chain (ancestral sampling), eta = 0 the deterministic (DDIM) chain."""
    s = one_minus_alphas_bar_sqrt.detach().cpu().double().reshape(-1)
    tau = [int(t) for t in timesteps]
    eta = float(eta)
    if not 0.0 <= eta <= 1.0:
        raise ValueError(f"eta must lie in [0, 1] (eta={eta})")
    if not tau or tau[0] < 0 or tau[-1] >= s.numel() or any(b <= a for a, b in zip(tau, tau[1:])):
        raise ValueError(f"timesteps must be a strictly increasing, non-empty subsequence of 0 .. {s.numel() - 1}, got {tau}")
    abar = (1.0 - s * s)[tau]
    coef = torch.zeros(len(tau), 4, dtype=torch.float64)
    a0 = abar[0]
    coef[0, 0], coef[0, 1], coef[0, 2] = 1 / a0.sqrt(), -(1 - a0.sqrt()) / a0.sqrt(), -(1 - a0).sqrt() / a0.sqrt()
    if len(tau) > 1:
        at, ar = abar[1:], abar[:-1]
        sigma = eta * torch.sqrt((1 - ar) / (1 - at)) * torch.sqrt(1 - at / ar)
        cy = torch.sqrt(ar / at)
        coef[1:, 0], coef[1:, 1] = cy, 1 - cy
        coef[1:, 2] = torch.sqrt(torch.clamp(1 - ar - sigma * sigma, min=0.0)) - cy * torch.sqrt(1 - at)
        coef[1:, 3] = sigma
    if not bool(torch.isfinite(coef).all()):
        raise ValueError("the schedule gives non-finite coefficients on these timesteps (abar = 0 or 1 somewhere)")
    return SamplerPlan(torch.tensor(tau, dtype=torch.int32), coef.float().contiguous())


def _engine_of(model):
    eng = getattr(model, "hip_engine", None)
    if eng is None:
        raise TypeError("model must be a nested_diffusion_amd.latent_model.ConditionalModel (HIP-backed)")
    return eng()


def p_sample(model, x, y, y_0_hat, y_T_mean, t, alphas, one_minus_alphas_bar_sqrt, output_detach=True, z=None):
    """Reverse step y_t -> y_{t-1} (diffusion_utils.py:54-92).  `z` (optional) replaces the internal
    torch.randn_like(y) draw."""
    eng = _engine_of(model)
    model.encode(x)
    eng.set_schedule(alphas, one_minus_alphas_bar_sqrt)
    if z is None:
        z = torch.randn_like(y)
    return eng.p_sample(0, y, y_0_hat, y_T_mean, int(t), z)


def p_sample_t_1to0(model, x, y, y_0_hat, y_T_mean, one_minus_alphas_bar_sqrt, output_detach=True):
    """diffusion_utils.py:96-111."""
    eng = _engine_of(model)
    model.encode(x)
    if eng._sched is None or eng._sched[1].numel() != one_minus_alphas_bar_sqrt.numel():
        eng.set_schedule(torch.ones_like(one_minus_alphas_bar_sqrt), one_minus_alphas_bar_sqrt)
    return eng.p_sample(0, y, y_0_hat, y_T_mean, 0, None)


def p_sample_loop(model, x, y_0_hat, y_T_mean, n_steps, alphas, one_minus_alphas_bar_sqrt, only_last_sample=False,
                  input_model_original_version=True, output_detach=True, noise: Optional[torch.Tensor] = None,
                  timesteps: Optional[Sequence[int]] = None, eta: float = 1.0) -> Union[torch.Tensor, List[torch.Tensor]]:
    """diffusion_utils.py:133-163.  Returns y_0 [B, C] when only_last_sample, else the list
    [y_T, y_{T-1}, ..., y_1, y_0] of n_steps + 1 tensors.

    noise: optional [n_steps, B, C] draws in the reference order (draw_reference_noise); when None the
    n_steps draws are made on y_T_mean's device with one torch.randn call.

    timesteps (not in the reference): an increasing subsequence of 0 .. n_steps-1 (timestep_sequence) to walk instead of every
    timestep, with the generalized update of sampler_plan at `eta`; the chain then has S = len(timesteps) steps: noise is [S, B, C]
    and the list has S + 1 entries.  The model's engine keeps no plan afterwards."""
    if not input_model_original_version:
        model = model.conditional_model
    eng = _engine_of(model)
    B, C = y_T_mean.shape
    plan = None
    if timesteps is not None:
        plan = sampler_plan(one_minus_alphas_bar_sqrt[:n_steps], timesteps, eta)
        n_steps = len(plan.timesteps)
    if noise is None:
        noise = torch.randn((n_steps, B, C), device=y_T_mean.device, dtype=torch.float32)
    elif tuple(noise.shape) != (n_steps, B, C):
        raise ValueError(f"noise must be [{n_steps}, {B}, {C}]")
    model.encode(x)
    eng.set_schedule(alphas, one_minus_alphas_bar_sqrt)
    dev = eng.device
    if plan is not None:
        eng.set_sampler(plan)
    try:
        out = eng.sample(y_0_hat.to(dev)[None], y_T_mean.to(dev)[None], noise.to(dev)[None], member0=0, n_members=1, mc=1,
                         T=n_steps, return_seq=not only_last_sample)
    finally:
        if plan is not None:
            eng.clear_sampler()
    if only_last_sample:
        return out[0]
    seq = list(out[0].unbind(0))
    assert len(seq) == n_steps + 1
    return seq
