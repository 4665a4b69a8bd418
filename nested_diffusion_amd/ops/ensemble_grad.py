"""What the input gradient through the sampler has beyond linear / linear_grad_input: the block product and its activation backward, the
reverse step and its backward, the aggregation's loss head and the softmax backward.  Binds csrc/nd_ensemble_grad.hip
(include/nested_diffusion.h: "the input gradient of the ensemble"; the chain: ensemble_grad.py)."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from .. import _lib
from .._lib import check, ptr
from ._base import _f32, _inplace, _labels, _on, _opt_f32, _stream

RSTEP_INIT, RSTEP_UPDATE, RSTEP_LAST = 0, 1, 2          # ND_RSTEP_*
RSTEP_MAX_C, RSTEP_MAX_LD = 8, 64
AGGREGATE_MAX_C = 16


def _rows(t: torch.Tensor, name: str, B: int) -> Tuple[int, int]:
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1 or B < 1 or t.shape[0] % B:
        raise ValueError(f"{name} must be [M, N] with M a positive multiple of B = {B} (shape {tuple(t.shape)})")
    return t.shape


def cond_mul(s: torch.Tensor, mul: torch.Tensor) -> torch.Tensor:
    """y[r] = s[r] * mul[r % B] (nd_cond_mul): s [M, N], mul [B, N], rows r = trial * B + image."""
    s, mul = _f32(s, "s"), _f32(mul, "mul")
    if mul.dim() != 2:
        raise ValueError("mul must be [B, N]")
    B = mul.shape[0]
    M, N = _rows(s, "s", B)
    _on(mul, "mul", (B, N), s.device)
    y = torch.empty_like(s)
    check(_lib.load().nd_cond_mul(ptr(s), ptr(mul), ptr(y), M, N, B, _stream(s)), "nd_cond_mul")
    return y


def cond_act_grad(dh: torch.Tensor, h: Optional[torch.Tensor], a_t: torch.Tensor, B: int, mul: Optional[torch.Tensor] = None,
                  dmul_acc: Optional[torch.Tensor] = None) -> torch.Tensor:
    """du [M, N] of one eval-mode ConditionalLinear + BatchNorm + softplus block (nd_cond_act_bwd) from dh = dL/d(its output) [M, N], the
    taped output h = softplus(z) (None: a block without activation), the scale row a_t [N] and, for the block whose output is multiplied by
    mul [B, N], that operand: dmul_acc [B, N] then receives + sum_trials dh * h IN PLACE.  B: images (rows r = trial * B + image)."""
    dh, a_t = _f32(dh, "dh"), _f32(a_t, "a_t")
    h, mul = _opt_f32(h, "h"), _opt_f32(mul, "mul")
    M, N = _rows(dh, "dh", B)
    _on(a_t, "a_t", (N,), dh.device)
    if h is not None:
        _on(h, "h", (M, N), dh.device)
    if (mul is None) != (dmul_acc is None) or (mul is not None and h is None):
        raise ValueError("mul, dmul_acc and the taped h come together")
    if mul is not None:
        _on(mul, "mul", (B, N), dh.device)
        _inplace(dmul_acc, "dmul_acc", torch.float32, (B, N))
    du = torch.empty_like(dh)
    check(_lib.load().nd_cond_act_bwd(ptr(dh), ptr(h), ptr(a_t), ptr(mul), ptr(du), ptr(dmul_acc), M, N, B, _stream(dh)), "nd_cond_act_bwd")
    return du


def reverse_step(mode: int, ymean: torch.Tensor, M: int, y: Optional[torch.Tensor] = None, eps: Optional[torch.Tensor] = None,
                 z: Optional[torch.Tensor] = None, alpha_t: float = 1.0, s_t: float = 0.0, s_tm1: float = 0.0, ld_out: Optional[int] = None
                 ) -> torch.Tensor:
    """One line of p_sample_loop on the [M, C] state (nd_reverse_step): RSTEP_INIT z + ymean, RSTEP_UPDATE p_sample's posterior,
    RSTEP_LAST p_sample_t_1to0.  ymean [B, C]; y [M, ld] (its first C columns are the state), eps, z [M, C]; alpha_t, s_t, s_tm1: the
    host's schedule entries.  ld_out (default C): 2C <= ld_out <= 64 writes lin1's input [y, ymean[r % B], 0 ..]."""
    ymean = _f32(ymean, "ymean")
    if ymean.dim() != 2:
        raise ValueError("ymean must be [B, C]")
    B, C = ymean.shape
    ldo = C if ld_out is None else int(ld_out)
    if mode not in (RSTEP_INIT, RSTEP_UPDATE, RSTEP_LAST):
        raise ValueError(f"unknown reverse-step mode {mode}")
    if not 1 <= C <= RSTEP_MAX_C or B < 1 or M < 1 or M % B or (ldo != C and not 2 * C <= ldo <= RSTEP_MAX_LD):
        raise ValueError(f"a reverse step takes 1 <= C <= {RSTEP_MAX_C}, M a positive multiple of B and ld_out == C or in [2C, {RSTEP_MAX_LD}] "
                         f"(M={M}, B={B}, C={C}, ld_out={ldo})")
    y, eps, z = _opt_f32(y, "y"), _opt_f32(eps, "eps"), _opt_f32(z, "z")
    if (mode != RSTEP_LAST and z is None) or (mode != RSTEP_INIT and (y is None or eps is None)):
        raise ValueError("INIT needs z; UPDATE needs y, eps and z; LAST needs y and eps")
    ldy = C
    if mode != RSTEP_INIT:
        if y.dim() != 2 or y.shape[0] != M or not C <= y.shape[1] <= RSTEP_MAX_LD or y.device != ymean.device:
            raise ValueError(f"y is {tuple(y.shape)}; expected [{M}, C <= ld <= {RSTEP_MAX_LD}] on {ymean.device}")
        ldy = y.shape[1]
        _on(eps, "eps", (M, C), ymean.device)
    if mode != RSTEP_LAST:
        _on(z, "z", (M, C), ymean.device)
    out = torch.empty(M, ldo, dtype=torch.float32, device=ymean.device)
    check(_lib.load().nd_reverse_step(mode, ptr(y) if mode != RSTEP_INIT else None, ldy, ptr(ymean), ptr(eps) if mode != RSTEP_INIT else None,
                                      ptr(z) if mode != RSTEP_LAST else None, ptr(out), ldo, M, B, C, float(alpha_t), float(s_t), float(s_tm1),
                                      _stream(ymean)), "nd_reverse_step")
    return out


def reverse_step_coef(ymean: torch.Tensor, y: torch.Tensor, eps: torch.Tensor, z: Optional[torch.Tensor], cy: float, cm: float, ce: float,
                      cz: float, ld_out: Optional[int] = None) -> torch.Tensor:
    """One step of a sampler plan on the [M, C] state (nd_reverse_step_coef): fmaf(cz, z, fmaf(ce, eps, fmaf(cm, ymean[r % B], cy * y))),
    the sampler's own device function.  Layouts as reverse_step: ymean [B, C], y [M, ld] (its first C columns), eps, z [M, C]; z None
    needs cz == 0 (the plan's row 0, or eta = 0).  ld_out (default C): 2C <= ld_out <= 64 writes lin1's input [y, ymean[r % B], 0 ..]."""
    ymean, y, eps, z = _f32(ymean, "ymean"), _f32(y, "y"), _f32(eps, "eps"), _opt_f32(z, "z")
    if ymean.dim() != 2 or y.dim() != 2:
        raise ValueError("ymean must be [B, C] and y [M, ld]")
    B, C = ymean.shape
    M = y.shape[0]
    ldo = C if ld_out is None else int(ld_out)
    if not 1 <= C <= RSTEP_MAX_C or B < 1 or M < 1 or M % B or (ldo != C and not 2 * C <= ldo <= RSTEP_MAX_LD):
        raise ValueError(f"a reverse step takes 1 <= C <= {RSTEP_MAX_C}, M a positive multiple of B and ld_out == C or in [2C, {RSTEP_MAX_LD}] "
                         f"(M={M}, B={B}, C={C}, ld_out={ldo})")
    if not C <= y.shape[1] <= RSTEP_MAX_LD or y.device != ymean.device:
        raise ValueError(f"y is {tuple(y.shape)}; expected [{M}, C <= ld <= {RSTEP_MAX_LD}] on {ymean.device}")
    _on(eps, "eps", (M, C), ymean.device)
    if z is None and float(cz) != 0.0:
        raise ValueError(f"cz = {cz} needs the draw z")
    if z is not None:
        _on(z, "z", (M, C), ymean.device)
    out = torch.empty(M, ldo, dtype=torch.float32, device=ymean.device)
    check(_lib.load().nd_reverse_step_coef(ptr(y), y.shape[1], ptr(ymean), ptr(eps), ptr(z), ptr(out), ldo, M, B, C, float(cy), float(cm),
                                           float(ce), float(cz), _stream(ymean)), "nd_reverse_step_coef")
    return out


def reverse_step_grad(g: torch.Tensor, C: int, cy: float, cm: float, ce: float, dymean: torch.Tensor, want_deps: bool = True,
                      ld_add: Optional[int] = None) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """The backward of one reverse step (nd_reverse_step_bwd) from g [M, ld]: its first C columns are dL/dy_{t-1}; with ld >= 2C its
    columns C .. 2C-1 (the yhat half of the gradient at lin1's input) join dymean too.  Returns (deps [M, C] = ce * g or None,
    dyadd [M, ld_add] = [cy * g, 0 ..] or None) and adds sum_trials (cm * g [+ the yhat half]) to dymean [B, C] IN PLACE."""
    g = _f32(g, "g")
    _inplace(dymean, "dymean", torch.float32)
    if dymean.dim() != 2 or dymean.shape[1] != C or not 1 <= C <= RSTEP_MAX_C:
        raise ValueError(f"dymean must be [B, C] with 1 <= C <= {RSTEP_MAX_C} (shape {tuple(dymean.shape)}, C={C})")
    B = dymean.shape[0]
    M, ldg = _rows(g, "g", B)
    if g.device != dymean.device or (ldg != C and not 2 * C <= ldg <= RSTEP_MAX_LD):
        raise ValueError(f"g is {tuple(g.shape)} on {g.device}: its row length must be C or in [2C, {RSTEP_MAX_LD}]")
    lda = C if ld_add is None else int(ld_add)
    if not C <= lda <= RSTEP_MAX_LD:
        raise ValueError(f"ld_add must lie in [C, {RSTEP_MAX_LD}] (ld_add={lda})")
    deps = torch.empty(M, C, dtype=torch.float32, device=g.device) if want_deps else None
    dyadd = torch.empty(M, lda, dtype=torch.float32, device=g.device) if ld_add is not None else None
    check(_lib.load().nd_reverse_step_bwd(ptr(g), ldg, float(cy), float(cm), float(ce), ptr(deps), ptr(dyadd), lda, ptr(dymean), M, B, C,
                                          _stream(g)), "nd_reverse_step_bwd")
    return deps, dyadd


def aggregate_xent_grad(samples: torch.Tensor, temperature: float, labels: Optional[torch.Tensor] = None, check_labels: bool = True):
    """(P [B, C], loss [B], dsamples [S, B, C]) of the ensemble's own loss (nd_aggregate_xent_bwd): samples [S, B, C] raw y_0,
    P = aggregate(samples, temperature)'s prob bit for bit, loss = -log P[b, label], dsamples = dloss / dsamples.  labels None:
    (P, None, None).  check_labels=False skips the label-range check, which reads back (the kernel gives an out-of-range label a NaN loss
    and no gradient)."""
    samples = _f32(samples, "samples")
    if samples.dim() != 3:
        raise ValueError("samples must be [S, B, C]")
    S, B, C = samples.shape
    if S < 1 or B < 1 or not 1 <= C <= AGGREGATE_MAX_C:
        raise ValueError(f"the aggregation takes S >= 1 samples, B >= 1 and 1 <= C <= {AGGREGATE_MAX_C} classes (S={S}, B={B}, C={C})")
    if not float(temperature) > 0.0:
        raise ValueError(f"temperature must be > 0 (temperature={temperature})")
    P = torch.empty(B, C, dtype=torch.float32, device=samples.device)
    loss = dsamples = None
    if labels is not None:
        labels = _labels(labels, samples.device, B, C if check_labels else None)
        loss = torch.empty(B, dtype=torch.float32, device=samples.device)
        dsamples = torch.empty_like(samples)
    check(_lib.load().nd_aggregate_xent_bwd(ptr(samples), ptr(labels), ptr(P), ptr(loss), ptr(dsamples), S, B, C, float(temperature),
                                            _stream(samples)), "nd_aggregate_xent_bwd")
    return P, loss, dsamples


def softmax_grad(p: torch.Tensor, dp: torch.Tensor) -> torch.Tensor:
    """dlogits = p * (dp - sum_c dp * p) over the last dim (nd_softmax_bwd): p = softmax(logits) and dp = dL/dp, any shape [..., C]."""
    p, dp = _f32(p, "p"), _f32(dp, "dp")
    if p.dim() < 1 or p.numel() < 1 or tuple(p.shape) != tuple(dp.shape) or p.device != dp.device:
        raise ValueError(f"p is {tuple(p.shape)} on {p.device}, dp {tuple(dp.shape)} on {dp.device}: expected one non-empty shape [..., C]")
    C = p.shape[-1]
    out = torch.empty_like(p)
    check(_lib.load().nd_softmax_bwd(ptr(p), ptr(dp), ptr(out), p.numel() // C, C, _stream(p)), "nd_softmax_bwd")
    return out
