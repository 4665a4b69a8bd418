"""The tail of a test run: softmax, aggregation over the samples, their statistics and the printed report.  Binds csrc/nd_report.hip
(include/nested_diffusion.h: "standalone operators" and "reporting tail of test_atk")."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from .. import _lib
from .._lib import check, ptr
from ._base import _f32, _i64, _stream


def softmax_rows(x: torch.Tensor) -> torch.Tensor:
    x = _f32(x, "x")
    C = x.shape[-1]
    out = torch.empty_like(x)
    check(_lib.load().nd_softmax_rows(ptr(x), ptr(out), x.numel() // C, C, _stream(x)), "nd_softmax_rows")
    return out


def aggregate(samples: torch.Tensor, temperature: float, return_probs: bool = False
              ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """samples [S, B, C] -> (prob [B, C], vote [B] int64, per-sample probs [S, B, C] or None).
    convert_to_prob + compute_ensemble_confidence + majority_voting_for_mc_samples
    (classification_train_separately.py:392-398, 425-447, 51-68)."""
    samples = _f32(samples, "samples")
    S, B, C = samples.shape
    prob = torch.empty(B, C, dtype=torch.float32, device=samples.device)
    vote = torch.empty(B, dtype=torch.int64, device=samples.device)
    probs = torch.empty_like(samples) if return_probs else None
    check(_lib.load().nd_aggregate(ptr(samples), ptr(prob), ptr(vote), ptr(probs), S, B, C, float(temperature), _stream(samples)),
          "nd_aggregate")
    return prob, vote, probs


def sample_stats(probs: torch.Tensor, q_lo: float = 0.025, q_hi: float = 0.975) -> Tuple[torch.Tensor, torch.Tensor]:
    """probs [S, B, C] -> (PIW [B, C] = quantile(q_hi) - quantile(q_lo) over S, unbiased variance [B, C]).
    compute_mean_piws_for_class :108-114, calculate_variances :166-172."""
    probs = _f32(probs, "probs")
    S, B, C = probs.shape
    piw = torch.empty(B, C, dtype=torch.float32, device=probs.device)
    var = torch.empty(B, C, dtype=torch.float32, device=probs.device)
    check(_lib.load().nd_sample_stats(ptr(probs), ptr(piw), ptr(var), S, B, C, float(q_lo), float(q_hi), _stream(probs)), "nd_sample_stats")
    return piw, var


def report(piw: torch.Tensor, var: torch.Tensor, prob_mean: torch.Tensor, vote: torch.Tensor, target: torch.Tensor,
           temperature: float, n_bins: int = 10) -> dict:
    """The numbers test_atk prints (classification_train_separately.py:801-838)."""
    piw, var, prob_mean = _f32(piw, "piw"), _f32(var, "var"), _f32(prob_mean, "prob_mean")
    N, C = prob_mean.shape
    vote, target = _i64(vote, piw.device), _i64(target, piw.device)
    out = torch.empty(2 + 4 * C, dtype=torch.float32, device=piw.device)
    check(_lib.load().nd_report(ptr(piw), ptr(var), ptr(prob_mean), ptr(vote), ptr(target), ptr(out), N, C, float(temperature), int(n_bins),
                                _stream(piw)), "nd_report")
    o = out.cpu()
    return {"accuracy": o[0], "ece": o[1], "piw_correct": o[2:2 + C], "piw_incorrect": o[2 + C:2 + 2 * C],
            "var_correct": o[2 + 2 * C:2 + 3 * C], "var_incorrect": o[2 + 3 * C:2 + 4 * C]}
