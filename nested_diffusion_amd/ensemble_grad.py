"""White-box attacks on the ensemble itself: the gradient of the ensemble's own loss with respect to the image, through the aggregation,
the K x mc reverse diffusions, the noise estimators' encoders and the conditioner.

The reference has the hook and never uses it: p_sample(..., output_detach=False) (diffusion/diffusion_utils.py:80-83, 103-106, 133-134).
The attacks it names (attack.Attack, L2Attack, autoattack.AutoAttack, CarliniWagner) craft their examples on the full ViT's head, and
mapping.ConditionerTarget attacks the mapping networks' averaged softmax; the probabilities Diffusion.test_atk reports come out of K
noise estimators run through a T-step reverse loop, each conditioned on yhat_k AND on the image (encoder_x reads it flattened).  This
module differentiates that: eval mode, guidance=True, arch 'linear', fp32.

Forward, per member k on rows r = trial * B + image (M = B * mc):
    yhat_k = softmax(mlp_k(prefix_k(x)));  xe_k = norm(encoder_x_k(x_flat));  y_T = z_0 + yhat_k
    t = T-1 .. 1:  eps = trunk_k(xe, y_t, t, yhat);  y_{t-1} = p_sample(y_t, yhat, eps, z)         then p_sample_t_1to0
    q_s = softmax(-(y0_s - 1)^2 / tau), s = k * mc + trial;  P = mean_s q_s;  loss[b] = -log P[b, label_b]
Backward (include/nested_diffusion.h lists every kernel's arithmetic): the aggregation head (ops.aggregate_xent_grad), then per member
the T steps in reverse -- a step is affine in (y_t, y_T_mean, eps) with the three coefficients of reverse_step_coefficients, the trunk
goes back through ops.linear_grad_input on the SAME packed weight images the forward streams and ops.cond_act_grad on the taped softplus
outputs -- then norm and encoder_x back to the flattened image, a softmax backward on yhat_k into the conditioner's own backward chain
(GuidingConditioner.backward), where the encoders' [B, D] gradient joins at the image.

What is taped: per member the three softplus outputs s1, h2, h3 [M, F] of every step (sigma(z) is recovered from them as -expm1(-h)),
xe and the encoder's two activations; the [M, C] states are not (the step is affine).  Summation orders: a step's sums over the trials run
in trial order inside one thread and are then added to what T - t earlier steps left (step order t = 0 .. T-1); the members' image
gradients are added in member order through linear_grad_input's `add`; P sums the samples s = 0 .. S-1 as ops.aggregate does.  No atomics:
the same call returns the same bits.

Memory: an EnsembleTarget holds its own packed copy of every selected member, K (D H + H^2 + H F + 2 F^2) 4 bytes (13.7 GB for K = 5 at
the config's D = 150528, H = F = 4096) plus the folded tables 6 T F 4 bytes per member; the tape is 3 M F 4 bytes per step and member
(0.8 GB for K = 5 at T = 100, B = 32, mc = 1) and a member's tape is freed step by step as its backward runs.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib, ops
from .diffusion_utils import sampler_plan, schedule_tables, timestep_sequence
from .latent_model import LIN1_K, check_member_dims, member_shapes, pad_lin1
from .mapping import require_fp32_split
from .ops import BN_EPS
from .ops._base import _labels

MAX_ROWS = ops.LINEAR_BWD_MAX_M


# ---- pure host functions (no GPU, no library) ---------------------------------------------------------------------------------------
def reverse_step_coefficients(alphas: torch.Tensor, one_minus_alphas_bar_sqrt: torch.Tensor) -> torch.Tensor:
    """[T, 3] float32: row t = (cy, cm, ce), the partial derivatives of the reverse step that leaves timestep t with respect to
    (y_t, y_T_mean, eps_theta).  t >= 1 is p_sample (diffusion_utils.py:68-92): with s = one_minus_alphas_bar_sqrt, sab = sqrt(1 - s_t^2)
    and gamma0, gamma1, gamma2 of :75-78, cy = gamma0 / sab + gamma1, cm = gamma2 - gamma0 (1 - sab) / sab, ce = -gamma0 s_t / sab;
    t = 0 is p_sample_t_1to0 (:99-111): cy = 1 / sab, cm = -(1 - sab) / sab, ce = -s_0 / sab.  Formed in double from the fp32 tables, as
    the trainer forms q_sample's, and rounded once."""
    a, s = alphas.detach().cpu().double().reshape(-1), one_minus_alphas_bar_sqrt.detach().cpu().double().reshape(-1)
    T = a.numel()
    if T < 1 or s.numel() != T:
        raise ValueError(f"alphas and one_minus_alphas_bar_sqrt must be two tables of one length T >= 1 (got {a.numel()} and {s.numel()})")
    out = torch.empty(T, 3, dtype=torch.float64)
    sab = torch.sqrt(1 - s * s)
    out[0] = torch.stack([1 / sab[0], -(1 - sab[0]) / sab[0], -s[0] / sab[0]])
    if T > 1:
        at, st, stm1, sabt, sabm = a[1:], s[1:], s[:-1], sab[1:], sab[:-1]
        g0 = (1 - at) * sabm / (st * st)
        g1 = (stm1 * stm1) * torch.sqrt(at) / (st * st)
        g2 = 1 + (sabt - 1) * (torch.sqrt(at) + sabm) / (st * st)
        out[1:, 0] = g0 / sabt + g1
        out[1:, 1] = g2 - g0 * (1 - sabt) / sabt
        out[1:, 2] = -g0 * st / sabt
    return out.float()


def member_dims(state_dict: Dict[str, torch.Tensor]) -> Tuple[int, int, int, int, int]:
    """(C, D, H, F, T) of a ConditionalModel state_dict (guidance=True, arch 'linear'), with every shape the chain relies on checked:
    D, H, F positive multiples of 16, 1 <= C <= 8, embedding tables of T + 1 >= 2 rows.  Raises KeyError / ValueError otherwise."""
    for _, key in _lib.MEMBER_WEIGHT_FIELDS:
        if key not in state_dict:
            raise KeyError(f"state_dict is missing '{key}'")
    sh = {k: tuple(v.shape) for k, v in state_dict.items()}
    H, D = sh["encoder_x.0.weight"]
    F = sh["encoder_x.6.weight"][0]
    C = sh["lin4.weight"][0]
    T = sh["lin1.embed.weight"][0] - 1
    for k, w in member_shapes(C, D, H, F, T).items():
        if sh[k] != w:
            raise ValueError(f"'{k}' has shape {sh[k]}, expected {w} (guidance=True, arch 'linear')")
    check_member_dims(C, D, H, F, T)
    return C, D, H, F, T


def check_call(B: int, mc: int, K: int, T: int, C: int, noise_shape: Optional[Sequence[int]]) -> int:
    """The per-call refusals of EnsembleTarget, as a pure function: M = B * mc.  One nd_linear_bwd launch takes 128 rows and the tape grows
    with M, so B * mc <= 128 (attack in smaller batches); a noise tensor must be [K, T, B * mc, C] in the reference's draw order."""
    M = B * mc
    if B < 1 or M > MAX_ROWS:
        raise ValueError(f"EnsembleTarget takes 1 <= B and B * mc <= {MAX_ROWS} rows per call (B={B}, mc={mc}): attack in smaller batches")
    if noise_shape is not None and tuple(noise_shape) != (K, T, M, C):
        raise ValueError(f"noise must be [{K}, {T}, {M}, {C}] (members, draws, B * mc rows r = trial * B + image, classes), got {list(noise_shape)}")
    return M


def _fold(sd: Dict[str, torch.Tensor], lin: str, bn: str, embed: Optional[str], T: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """nd_load_member's folds (csrc/nd_handle.hip) in double, rounded once: eval BatchNorm(g_t (W h + b)) = a_t (W h) + c_t with
    s = w / sqrt(var + 1e-5), a_t = s g_t, c_t = s g_t b + (beta - mean s).  embed None: g = 1, one row."""
    d = lambda k: sd[k].detach().double()                                     # noqa: E731
    s = d(bn + ".weight") / torch.sqrt(d(bn + ".running_var") + BN_EPS)
    o = d(bn + ".bias") - d(bn + ".running_mean") * s
    g = d(embed)[:T] if embed is not None else torch.ones(1, s.numel(), dtype=torch.float64, device=s.device)
    a = s[None, :] * g
    c = a * d(lin + ".bias")[None, :] + o[None, :]
    return a.float().contiguous(), c.float().contiguous()


# ---- one member ---------------------------------------------------------------------------------------------------------------------
class SamplerTape:
    """One noise estimator (ConditionalModel, guidance=True, arch 'linear') in eval mode with the tape of its last forward:
    forward(x_flat, yhat, noise) -> y0 [M, C], backward(dy0) -> (dx_flat [B, D], dyhat [B, C]).  The seven Linear weights are held as
    ops.PackedWeight images (lin1 padded to LIN1_K columns), BatchNorm, bias and the per-timestep gain folded into [T, F] tables once,
    here (torch arithmetic in double: load time).  y_T_mean and y_0_hat are the same tensor yhat.  Accepted shapes: D, H, F
    positive multiples of 16, 1 <= C <= 8, T >= 1 (T = 1 is the p_sample_t_1to0-only chain).

    timesteps (default None: every timestep, the reference's chain): a sampler plan (diffusion_utils.sampler_plan(.., timesteps, eta)) --
    the chain then has S = len(timesteps) steps, position j evaluating eps at timestep timesteps[j]; its forward goes through
    ops.reverse_step_coef (the sampler's own device function), its backward uses (cy, cm, ce) of the same plan, noise is [S, M, C] and
    the tape holds S steps."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], alphas: torch.Tensor, one_minus_alphas_bar_sqrt: torch.Tensor, device="cuda",
                 timesteps: Optional[Sequence[int]] = None, eta: float = 1.0):
        self.C, self.D, self.H, self.F, T_emb = member_dims(state_dict)
        self.coef = reverse_step_coefficients(alphas, one_minus_alphas_bar_sqrt).tolist()
        self.T = len(self.coef)
        if self.T > T_emb:
            raise ValueError(f"the schedule has {self.T} timesteps, the embedding tables {T_emb}")
        self.plan = None if timesteps is None else sampler_plan(one_minus_alphas_bar_sqrt, timesteps, eta)
        if self.plan is not None:
            self.coef = self.plan.coef.tolist()                                 # rows (cy, cm, ce, cz); the backward reads the first three
        self.rows = list(range(self.T)) if self.plan is None else self.plan.timesteps.tolist()    # chain position j -> timestep
        self.S = len(self.rows)
        self.alphas = alphas.detach().cpu().float().reshape(-1).tolist()
        self.omabs = one_minus_alphas_bar_sqrt.detach().cpu().float().reshape(-1).tolist()
        self.device = torch.device(device)
        sd = {k: v.detach().to(self.device, torch.float32) for k, v in state_dict.items() if v.is_floating_point()}
        self.w = {"enc0": ops.PackedWeight(sd["encoder_x.0.weight"].contiguous()), "enc3": ops.PackedWeight(sd["encoder_x.3.weight"].contiguous()),
                  "enc6": ops.PackedWeight(sd["encoder_x.6.weight"].contiguous()), "lin1": ops.PackedWeight(pad_lin1(sd["lin1.lin.weight"])),
                  "lin2": ops.PackedWeight(sd["lin2.lin.weight"].contiguous()), "lin3": ops.PackedWeight(sd["lin3.lin.weight"].contiguous()),
                  "lin4": ops.PackedWeight(sd["lin4.weight"].contiguous())}
        self.b4 = sd["lin4.bias"].contiguous()
        self.a, self.c = {}, {}
        for name, lin, bn, emb in (("enc0", "encoder_x.0", "encoder_x.1", None), ("enc3", "encoder_x.3", "encoder_x.4", None),
                                   ("enc6", "encoder_x.6", "norm", None), ("lin1", "lin1.lin", "unetnorm1", "lin1.embed.weight"),
                                   ("lin2", "lin2.lin", "unetnorm2", "lin2.embed.weight"), ("lin3", "lin3.lin", "unetnorm3", "lin3.embed.weight")):
            self.a[name], self.c[name] = _fold(sd, lin, bn, emb, self.T)
        self._tape = None

    def _check(self, x_flat, yhat, noise) -> Tuple[int, int]:
        for t, name in ((x_flat, "x_flat"), (yhat, "yhat"), (noise, "noise")):
            ops._f32(t, name)
        if x_flat.dim() != 2 or x_flat.shape[1] != self.D or x_flat.shape[0] < 1:
            raise ValueError(f"x_flat must be [B, {self.D}], got {tuple(x_flat.shape)}")
        B = x_flat.shape[0]
        if tuple(yhat.shape) != (B, self.C):
            raise ValueError(f"yhat must be [{B}, {self.C}], got {tuple(yhat.shape)}")
        if noise.dim() != 3 or noise.shape[0] != self.S or noise.shape[2] != self.C or noise.shape[1] < B or noise.shape[1] % B:
            raise ValueError(f"noise must be [{self.S}, B * mc, {self.C}] with B = {B}, got {tuple(noise.shape)}")
        return B, noise.shape[1]

    def forward(self, x_flat: torch.Tensor, yhat: torch.Tensor, noise: torch.Tensor, record: bool = True) -> torch.Tensor:
        """y0 [M, C] of p_sample_loop (diffusion_utils.py:133-163) with noise [T, M, C] in the reference's draw order: row 0 the initial
        draw, row i the draw of p_sample at t = T - i (with a plan: [S, M, C], row i the draw of the step that leaves chain position
        S - i).  record=False keeps no tape (EnsembleTarget.forward)."""
        B, M = self._check(x_flat, yhat, noise)
        w, a, c, T = self.w, self.a, self.c, self.S
        x_flat, yhat, noise = x_flat.contiguous(), yhat.contiguous(), noise.contiguous()
        e0 = ops.linear(x_flat, w["enc0"], c["enc0"][0], act="softplus", scale=a["enc0"][0])
        e1 = ops.linear(e0, w["enc3"], c["enc3"][0], act="softplus", scale=a["enc3"][0])
        xe = ops.linear(e1, w["enc6"], c["enc6"][0], scale=a["enc6"][0])
        inp = ops.reverse_step(ops.RSTEP_INIT, yhat, M, z=noise[0], ld_out=LIN1_K)
        steps: List[Optional[tuple]] = [None] * T
        y0 = None
        for j in range(T - 1, -1, -1):
            t = self.rows[j]
            s1 = ops.linear(inp, w["lin1"], c["lin1"][t], act="softplus", scale=a["lin1"][t])
            h2 = ops.linear(ops.cond_mul(s1, xe), w["lin2"], c["lin2"][t], act="softplus", scale=a["lin2"][t])
            h3 = ops.linear(h2, w["lin3"], c["lin3"][t], act="softplus", scale=a["lin3"][t])
            eps = ops.linear(h3, w["lin4"], self.b4)
            if self.plan is not None:
                if j >= 1:
                    inp = ops.reverse_step_coef(yhat, inp, eps, noise[T - j], *self.coef[j], ld_out=LIN1_K)
                else:
                    y0 = ops.reverse_step_coef(yhat, inp, eps, None, *self.coef[0])
            elif t >= 1:
                inp = ops.reverse_step(ops.RSTEP_UPDATE, yhat, M, y=inp, eps=eps, z=noise[T - t], alpha_t=self.alphas[t], s_t=self.omabs[t],
                                       s_tm1=self.omabs[t - 1], ld_out=LIN1_K)
            else:
                y0 = ops.reverse_step(ops.RSTEP_LAST, yhat, M, y=inp, eps=eps, s_t=self.omabs[0])
            if record:
                steps[j] = (s1, h2, h3)
        self._tape = dict(B=B, M=M, e0=e0, e1=e1, xe=xe, steps=steps) if record else None
        return y0

    def backward(self, dy0: torch.Tensor, add: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(dx_flat [B, D], dyhat [B, C]) from dy0 = dL/dy0 [M, C] of the last recorded forward; add [B, D] joins dx_flat (the members'
        image gradients are summed this way, in call order).  The tape is used up: every step's activations are released behind it."""
        tape = self._tape
        if tape is None:
            raise RuntimeError("SamplerTape.backward needs a recorded forward (each tape serves one backward)")
        self._tape = None
        B, M, C = tape["B"], tape["M"], self.C
        dy0 = ops._f32(dy0, "dy0")
        if tuple(dy0.shape) != (M, C):
            raise ValueError(f"dy0 is {tuple(dy0.shape)}; expected {[M, C]}")
        w, a, xe, steps = self.w, self.a, tape["xe"], tape["steps"]
        dyhat = torch.zeros(B, C, dtype=torch.float32, device=self.device)
        dxe = torch.zeros(B, self.F, dtype=torch.float32, device=self.device)
        g = dy0
        for j in range(self.S):
            t = self.rows[j]
            cy, cm, ce = self.coef[j][:3]
            deps, dyadd = ops.reverse_step_grad(g, C, cy, cm, ce, dyhat, ld_add=LIN1_K)
            s1, h2, h3 = steps[j]
            du3 = ops.cond_act_grad(ops.linear_grad_input(deps, w["lin4"]), h3, a["lin3"][t], B)
            du2 = ops.cond_act_grad(ops.linear_grad_input(du3, w["lin3"]), h2, a["lin2"][t], B)
            du1 = ops.cond_act_grad(ops.linear_grad_input(du2, w["lin2"]), s1, a["lin1"][t], B, mul=xe, dmul_acc=dxe)
            g = ops.linear_grad_input(du1, w["lin1"], add=dyadd)               # [M, 16]: dL/dy_t, the yhat half, zeros
            steps[j] = None
        ops.reverse_step_grad(g, C, 0.0, 1.0, 0.0, dyhat, want_deps=False)      # y_T = z_0 + yhat, and the last yhat half
        dn = ops.cond_act_grad(dxe, None, a["enc6"][0], B)
        du1 = ops.cond_act_grad(ops.linear_grad_input(dn, w["enc6"]), tape["e1"], a["enc3"][0], B)
        du0 = ops.cond_act_grad(ops.linear_grad_input(du1, w["enc3"]), tape["e0"], a["enc0"][0], B)
        return ops.linear_grad_input(du0, w["enc0"], add=add), dyhat


# ---- the attacks' model ---------------------------------------------------------------------------------------------------------------
def check_target_args(conditioner, states, mc: int, members) -> List[int]:
    """Every refusal of EnsembleTarget's constructor, before anything is packed or launched: the selected members."""
    require_fp32_split("EnsembleTarget", mlps=conditioner.mlps)              # nothing built here yet: the environment counts
    require_fp32_split("EnsembleTarget", vit=conditioner.vit)
    if int(mc) < 1:
        raise ValueError(f"mc must be at least 1 (mc={mc})")
    members = conditioner._members(members if members is not None else range(min(len(states), len(conditioner.mlps))))
    missing = [k for k in members if k >= len(states) or states[k] is None]
    if missing:
        raise ValueError(f"no noise estimator state for member(s) {missing}: member k is conditioned on mapping MLP k and needs states[k]")
    return members


class EnsembleTarget:
    """What the gradient attacks take as their model when the ENSEMBLE is attacked end to end (duck-typed like mapping.ConditionerTarget):
    .device, forward(x) -> P [B, C], the ensemble's probabilities (compute_ensemble_confidence, what test_atk reports), and
    input_grad(x, labels, noise=None) -> (P, dx, loss) with loss[b] = -log P[b, label_b] and dx = d(loss.sum()) / dx [B, 3, H, W].  It has
    no attribute called `vit` (attack._vit would unwrap it).

    states[k]: member k's ConditionalModel state_dict (the checkpoint's 'noise_estimator'); member k is conditioned on mapping MLP k.
    members (default: every member that has a state and an MLP) selects as ConditionerTarget does.  noise [len(members), T, B * mc, C] in the
    reference's draw order, as Diffusion.predict_batch takes it; None draws fresh noise on EVERY call from (seed, a call counter), so an
    iterative attack averages over the defence's randomness across its steps (expectation over transformation); fix_noise() pins one
    sample path instead.  Refused, before anything is launched: the fp16 mode, ND_GEMM_F32=mfma_f32, B * mc > 128, a noise tensor of the
    wrong shape.  The module docstring states the memory this holds.

    sample_steps (default None: every timestep of the config's schedule): attack the ensemble as it is run with a sampler plan of
    timestep_sequence(T, sample_steps, skip_type) at `eta` (diffusion_utils.sampler_plan; main --sample_steps): every chain has
    S = self.steps steps, in time and in tape, and noise is [len(members), S, B * mc, C]."""

    def __init__(self, conditioner, states: Sequence[Optional[Dict[str, torch.Tensor]]], config, mc: int = 1,
                 members: Optional[Sequence[int]] = None, temperature: Optional[float] = None, seed: int = 0,
                 sample_steps: Optional[int] = None, skip_type: str = "uniform", eta: float = 1.0):
        self.members = check_target_args(conditioner, states, mc, members)
        timesteps = None if sample_steps is None else timestep_sequence(int(config.diffusion.timesteps), sample_steps, skip_type)
        if not 0.0 <= float(eta) <= 1.0:
            raise ValueError(f"eta must lie in [0, 1] (eta={eta})")
        self.cond, self.mc, self.seed = conditioner, int(mc), int(seed)
        self.device = conditioner.vit.device
        if temperature is None:
            from .runner import temperature_for
            temperature = temperature_for(config.data.dataset)
        self.temperature = float(temperature)
        if not self.temperature > 0.0:
            raise ValueError(f"temperature must be > 0 (temperature={temperature})")
        self.T = int(config.diffusion.timesteps)
        tables = schedule_tables(config.diffusion.beta_schedule, self.T, config.diffusion.beta_start, config.diffusion.beta_end)
        dims = [member_dims(states[k]) for k in self.members]
        want = (int(config.data.num_classes), int(config.model.data_dim), int(config.model.hidden_dim), int(config.model.feature_dim))
        for k, d in zip(self.members, dims):
            if d[:4] != want or d[4] < self.T:
                raise ValueError(f"member {k} has (C, D, H, F, T) = {d}; the config says {want} and {self.T} timesteps")
        self.C, self.D = want[0], want[1]
        self.tapes = [SamplerTape(states[k], tables.alphas, tables.one_minus_alphas_bar_sqrt, self.device, timesteps=timesteps, eta=eta)
                      for k in self.members]
        self.steps = self.T if timesteps is None else len(timesteps)         # reverse steps (and draws) per chain
        self._calls = 0
        self._fixed: Optional[torch.Tensor] = None

    # -- noise ------------------------------------------------------------------------------------------------------------------------
    def draw_noise(self, B: int, counter: Optional[int] = None) -> torch.Tensor:
        """[len(members), T, B * mc, C] standard normals from (seed, counter); counter None: the call counter, which then advances."""
        if counter is None:
            counter, self._calls = self._calls, self._calls + 1
        gen = torch.Generator(device=self.device)
        gen.manual_seed((self.seed * 1000003 + int(counter)) & 0x7FFFFFFFFFFFFFFF)
        return torch.randn(len(self.members), self.steps, B * self.mc, self.C, dtype=torch.float32, device=self.device, generator=gen)

    def fix_noise(self, noise: Optional[torch.Tensor] = None, B: Optional[int] = None) -> torch.Tensor:
        """Pin one sample path: every later call without a noise argument uses `noise` (or, given B, a draw from (seed, counter 0) made
        now) until free_noise().  Returns the pinned tensor."""
        if noise is None:
            if B is None:
                raise ValueError("fix_noise needs a noise tensor or the batch size B to draw one for")
            noise = self.draw_noise(B, counter=0)
        self._fixed = ops._f32(noise, "noise")
        return self._fixed

    def free_noise(self) -> None:
        self._fixed = None

    def _noise(self, B: int, noise: Optional[torch.Tensor]) -> torch.Tensor:
        if noise is None:
            noise = self._fixed
        check_call(B, self.mc, len(self.members), self.steps, self.C, None if noise is None else noise.shape)
        return self.draw_noise(B) if noise is None else ops._f32(noise, "noise")

    # -- the chain ----------------------------------------------------------------------------------------------------------------------
    def _image(self, x: torch.Tensor) -> torch.Tensor:
        x = ops._f32(x, "x")
        if x.dim() != 4 or x[0].numel() != self.D:
            raise ValueError(f"x must be [B, Cin, H, W] with Cin * H * W = {self.D}, got {tuple(x.shape)}")
        return x

    def _samples(self, x: torch.Tensor, yhat: torch.Tensor, noise: torch.Tensor, record: bool) -> torch.Tensor:
        """[K * mc, B, C]: member-major then trial, as test_atk stacks them (classification_train_separately.py:767-777)."""
        B = x.shape[0]
        x_flat = x.reshape(B, self.D)
        y0 = [tape.forward(x_flat, yhat[i], noise[i], record=record) for i, tape in enumerate(self.tapes)]
        return torch.stack(y0).reshape(len(self.tapes) * self.mc, B, self.C)

    def forward(self, x: torch.Tensor, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """P [B, C].  Without a noise argument (and no pinned path) every call draws anew: the defence is stochastic."""
        x = self._image(x)
        noise = self._noise(x.shape[0], noise)
        out = self.cond.compute_guiding_prediction(x, include_full_vit=False)
        yhat = ops.softmax_rows(torch.stack([out[k] for k in self.members]))
        return ops.aggregate_xent_grad(self._samples(x, yhat, noise, record=False), self.temperature)[0]

    __call__ = forward

    def input_grad(self, x: torch.Tensor, labels: torch.Tensor, noise: Optional[torch.Tensor] = None, check_labels: bool = True
                   ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        x = self._image(x)
        B = x.shape[0]
        noise = self._noise(B, noise)
        labels = _labels(labels, x.device, B, self.C if check_labels else None)
        logits, ctape = self.cond.forward_recorded(x, self.members)
        yhat = ops.softmax_rows(logits)
        samples = self._samples(x, yhat, noise, record=True)
        P, loss, dsamples = ops.aggregate_xent_grad(samples, self.temperature, labels, check_labels=False)
        dsamples = dsamples.reshape(len(self.tapes), B * self.mc, self.C)
        dx_flat, dyhat = None, []
        for i, tape in enumerate(self.tapes):                                  # member order: the image gradients' summation order
            dx_flat, dy = tape.backward(dsamples[i], add=dx_flat)
            dyhat.append(dy)
        dlogits = ops.softmax_grad(yhat, torch.stack(dyhat))
        return P, self.cond.backward(ctape, dlogits, add=dx_flat), loss

    def input_grad_margin(self, *args, **kwargs):
        raise NotImplementedError("Carlini-Wagner (CarliniWagner) is not implemented on an EnsembleTarget: its margin loss is defined on the "
                                  "full ViT's logits, not on the ensemble's aggregated probabilities")
