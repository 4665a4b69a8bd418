"""The training step of the noise estimators: BatchNorm forward / backward, q_sample, the MSE loss, and clip + Adam on materialised
gradients.  Binds csrc/nd_diffusion_train.hip (include/nested_diffusion.h: "training of the noise estimators"; the loop:
train_diffusion.py)."""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from .. import _lib
from .._lib import ND_ACT_NONE, ND_ACT_SOFTPLUS, check, ptr
from ._base import _f32, _inplace, _on, _opt_f32, _stream, _workspace
from .packed_linear import LINEAR_BWD_MAX_M, PackedWeight

BN_EPS, BN_MOMENTUM = 1e-5, 0.1                           # nn.BatchNorm1d's defaults (latent_model.py:129-166)
SUMSQ_CHUNK = 4096                                         # ND_SUMSQ_CHUNK: floats per first-stage partial of nd_sumsq
_BN_ACT = {"none": ND_ACT_NONE, None: ND_ACT_NONE, "softplus": ND_ACT_SOFTPLUS}


def _bn_args(what: str, u: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, table, t, mul, act):
    """The checks nd_bn_train_fwd and nd_bn_train_bwd share: (M, N, table, t, mul, act code, rows_table)."""
    if act not in _BN_ACT:
        raise ValueError(f"{what}: act must be None or 'softplus' (act={act!r})")
    if u.dim() != 2 or not 2 <= u.shape[0] <= LINEAR_BWD_MAX_M or u.shape[1] < 1:
        raise ValueError(f"{what}: expected [2 <= M <= {LINEAR_BWD_MAX_M}, N >= 1], got {tuple(u.shape)} (batch statistics need two rows)")
    M, N = u.shape
    _on(gamma, "gamma", (N,), u.device)
    _on(beta, "beta", (N,), u.device)
    if (table is None) != (t is None):
        raise ValueError(f"{what}: table and t come together")
    rows_table = 0
    if table is not None:
        table = _f32(table, "table")
        if table.dim() != 2 or table.shape[0] < 1 or table.shape[1] != N or table.device != u.device:      # any row count: not _on
            raise ValueError(f"table is {tuple(table.shape)} on {table.device}; expected [rows >= 1, {N}] on {u.device}")
        if not t.is_cuda or t.dtype != torch.int32 or tuple(t.shape) != (M,) or t.device != u.device:
            raise ValueError(f"t must be an int32 GPU tensor [{M}] on {u.device} (checked against the table on the host before the upload)")
        t, rows_table = t.contiguous(), table.shape[0]
    if mul is not None:
        mul = _f32(mul, "mul")
        _on(mul, "mul", (M, N), u.device)
    return M, N, table, t, mul, _BN_ACT[act], rows_table


def bn_train_forward(u: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, table: Optional[torch.Tensor] = None,
                     t: Optional[torch.Tensor] = None, mul: Optional[torch.Tensor] = None, act=None,
                     running_mean: Optional[torch.Tensor] = None, running_var: Optional[torch.Tensor] = None, eps: float = BN_EPS,
                     momentum: float = BN_MOMENTUM) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(out [M, N], xhat [M, N], rstd [N]) of act(BatchNorm1d_train(table[t] * u)) * mul (nd_bn_train_fwd): u the Linear's output,
    table [rows, N] with t [M] int32 the ConditionalLinear gain (or both None), mul [M, N] or None, act None or 'softplus'.
    running_mean / running_var [N], if given, are updated IN PLACE as torch does (momentum, unbiased variance).  2 <= M <= 128.
    t must have been checked against the table on the host: a row outside it gets gain 0."""
    u, gamma, beta = _f32(u, "u"), _f32(gamma, "gamma"), _f32(beta, "beta")
    M, N, table, t, mul, code, rows_table = _bn_args("bn_train_forward", u, gamma, beta, table, t, mul, act)
    if eps < 0.0:
        raise ValueError(f"bn_train_forward needs eps >= 0 (eps={eps})")
    rm, rv = _inplace(running_mean, "running_mean", shape=(N,)), _inplace(running_var, "running_var", shape=(N,))
    if (rm is None) != (rv is None) or (rm is not None and (rm.data_ptr() == rv.data_ptr() or rm.device != u.device or rv.device != u.device)):
        raise ValueError("running_mean and running_var come together, as two buffers on u's device")
    out, xhat = torch.empty_like(u), torch.empty_like(u)
    rstd = torch.empty(N, dtype=torch.float32, device=u.device)
    check(_lib.load().nd_bn_train_fwd(ptr(u), ptr(table), ptr(t), rows_table, ptr(mul), ptr(gamma), ptr(beta), ptr(out), ptr(xhat), ptr(rstd),
                                      ptr(rm), ptr(rv), M, N, code, float(eps), float(momentum), _stream(u)), "nd_bn_train_fwd")
    return out, xhat, rstd


def bn_train_backward(dout: torch.Tensor, xhat: torch.Tensor, rstd: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
                      u: Optional[torch.Tensor] = None, table: Optional[torch.Tensor] = None, t: Optional[torch.Tensor] = None,
                      mul: Optional[torch.Tensor] = None, act=None, want_dmul: bool = False) -> dict:
    """The gradient of bn_train_forward given dout = dL/d(out) and the forward's xhat, rstd (nd_bn_train_bwd): a dict with du [M, N],
    dgamma [N], dbeta [N], and -- with the gain (u, table, t as in the forward) -- dtable, the DENSE [rows, N] gradient of the table
    (rows whose index does not occur are exactly 0), and -- with mul and want_dmul -- dmul [M, N]."""
    dout, xhat, rstd, gamma, beta = _f32(dout, "dout"), _f32(xhat, "xhat"), _f32(rstd, "rstd"), _f32(gamma, "gamma"), _f32(beta, "beta")
    M, N, table, t, mul, code, rows_table = _bn_args("bn_train_backward", dout, gamma, beta, table, t, mul, act)
    _on(xhat, "xhat", (M, N), dout.device)
    _on(rstd, "rstd", (N,), dout.device)
    if table is not None:
        if u is None:
            raise ValueError("bn_train_backward: the gain needs u, the Linear's output")
        u = _f32(u, "u")
        _on(u, "u", (M, N), dout.device)
    else:
        u = None
    if want_dmul and mul is None:
        raise ValueError("bn_train_backward: want_dmul without mul")
    dev = dout.device
    res = {"du": torch.empty_like(dout), "dgamma": torch.empty(N, dtype=torch.float32, device=dev),
           "dbeta": torch.empty(N, dtype=torch.float32, device=dev)}
    if table is not None:
        res["dtable"] = torch.empty(rows_table, N, dtype=torch.float32, device=dev)      # zeroed by the entry point, on the stream
    if want_dmul:
        res["dmul"] = torch.empty_like(dout)
    check(_lib.load().nd_bn_train_bwd(ptr(dout), ptr(u), ptr(table), ptr(t), rows_table, ptr(mul), ptr(xhat), ptr(rstd), ptr(gamma), ptr(beta),
                                      ptr(res["du"]), ptr(res.get("dmul")), ptr(res["dgamma"]), ptr(res["dbeta"]), ptr(res.get("dtable")), M, N,
                                      code, _stream(dout)), "nd_bn_train_bwd")
    return res


def _rows_by_classes(what: str, tensors) -> Tuple[int, int]:
    first = tensors[0][0]
    if first.dim() != 2:
        raise ValueError(f"{what}: {tensors[0][1]} must be [M, C]")
    M, C = first.shape
    if not 1 <= M <= LINEAR_BWD_MAX_M or not 1 <= C <= 1024:
        raise ValueError(f"{what} takes 1 <= M <= {LINEAR_BWD_MAX_M} rows and 1 <= C <= 1024 classes (M={M}, C={C})")
    for p, name in tensors[1:]:
        _on(p, name, (M, C), first.device)
    return M, C


def qsample(y0: torch.Tensor, yhat: torch.Tensor, e: torch.Tensor, ca: torch.Tensor, cb: torch.Tensor) -> torch.Tensor:
    """q_sample with per-row coefficients gathered on the HOST (nd_qsample): ca[r] * y0 + (1 - ca[r]) * yhat + cb[r] * e; y0, yhat, e
    [M, C], ca = alphas_bar_sqrt[t], cb = one_minus_alphas_bar_sqrt[t] as float32 [M]."""
    y0, yhat, e, ca, cb = _f32(y0, "y0"), _f32(yhat, "yhat"), _f32(e, "e"), _f32(ca, "ca"), _f32(cb, "cb")
    M, C = _rows_by_classes("qsample", ((y0, "y0"), (yhat, "yhat"), (e, "e")))
    _on(ca, "ca", (M,), y0.device)
    _on(cb, "cb", (M,), y0.device)
    yt = torch.empty_like(y0)
    check(_lib.load().nd_qsample(ptr(y0), ptr(yhat), ptr(e), ptr(ca), ptr(cb), ptr(yt), M, C, _stream(y0)), "nd_qsample")
    return yt


def mse_grad(out: torch.Tensor, e: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(loss, dout) of loss = (e - out).square().mean() (nd_mse_grad): loss a device scalar summed in row-major order, dout = dloss/dout
    = (out - e) * 2 / (M * C)."""
    out, e = _f32(out, "out"), _f32(e, "e")
    M, C = _rows_by_classes("mse_grad", ((out, "out"), (e, "e")))
    dout = torch.empty_like(out)
    loss = torch.empty((), dtype=torch.float32, device=out.device)
    check(_lib.load().nd_mse_grad(ptr(out), ptr(e), ptr(dout), ptr(loss), M, C, _stream(out)), "nd_mse_grad")
    return loss, dout


def sumsq_plan(n: int) -> dict:
    """The summation order of nd_sumsq for n floats (host only): first-stage chunks and the longest serial chain of additions."""
    out = (ctypes.c_size_t * 2)()
    check(_lib.load().nd_sumsq_plan(int(n), out), "nd_sumsq_plan")
    return {"chunks": int(out[0]), "chain": int(out[1])}


def sumsq(x, acc: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """acc[0] (+)= sum of x's squares (nd_sumsq), x a float32 GPU tensor or a PackedWeight image (its zero padding adds nothing).  acc: a
    float32 GPU scalar written in place (made if None); accumulate: add to what it holds.  The order depends on x.numel() alone."""
    x = _f32(x.data if isinstance(x, PackedWeight) else x, "x")
    n = x.numel()
    if n < 1:
        raise ValueError("sumsq of an empty tensor")
    if acc is None:
        if accumulate:
            raise ValueError("sumsq: accumulate needs acc")
        acc = torch.empty((), dtype=torch.float32, device=x.device)
    _inplace(acc, "acc")
    if acc.numel() != 1 or acc.device != x.device:
        raise ValueError(f"acc must be one float32 on {x.device}")
    lib = _lib.load()
    ws = _workspace(lib.nd_sumsq_workspace_bytes(n), x.device)
    check(lib.nd_sumsq(ptr(x), n, ptr(acc), 1 if accumulate else 0, ptr(ws), ws.numel(), _stream(x)), "nd_sumsq")
    return acc


def clip_adam(w, m, v, g, adam, sumsq: Optional[torch.Tensor] = None, max_norm: float = 1.0, shadow=None, ema=None) -> None:
    """clip_grad_norm_'s scaling by min(1, max_norm / (sqrt(sumsq) + 1e-6)) and one Adam step on a materialised gradient, in place on w,
    m, v (nd_clip_adam).  w, m, v, g: four float32 GPU tensors of one shape, or four PackedWeight images of one shape (elementwise: the
    layout does not matter).  sumsq: the device scalar ops.sumsq accumulated over ALL gradients, or None for no clipping.
    shadow with ema = ops.ema_step(mu): the same pass also moves the EMA shadow of w towards the new weight, in place
    (nd_clip_adam_ema: shadow = (1 - mu) * w_new + mu * shadow); shadow obeys m's and v's rules and is a fifth distinct buffer (a packed
    image's zero padding stays zero).  Both come together; neither: nd_clip_adam as it always was."""
    if not isinstance(adam, _lib.NdAdamStep):
        raise TypeError("adam must be an ops.adam_step(...)")
    if (shadow is None) != (ema is None):
        raise ValueError("clip_adam: shadow and ema come together (ema = ops.ema_step(mu))")
    if ema is not None and not isinstance(ema, _lib.NdEmaStep):
        raise TypeError("ema must be an ops.ema_step(...)")
    state = ((m, "m"), (v, "v")) + (((shadow, "shadow"),) if ema is not None else ())
    if isinstance(w, PackedWeight):
        for p, name in state + ((g, "g"),):
            if not isinstance(p, PackedWeight) or (p.N, p.K, p.dtype) != (w.N, w.K, w.dtype):
                raise ValueError(f"{name} must be a PackedWeight image of w's shape [{w.N}, {w.K}]")
        if w.dtype != _lib.ND_DTYPE_F32:
            raise _lib.NdError("clip_adam updates fp32 weight images only")
        w, g = w.data, g.data
        state = tuple((p.data, name) for p, name in state)
    elif isinstance(shadow, PackedWeight):
        raise ValueError("shadow is a PackedWeight image, w a tensor: the five buffers are tensors or images alike")
    g = _f32(g, "g")
    state = ((w, "w"),) + state
    for p, name in state:
        _inplace(p, name, shape=tuple(g.shape))
        if p.device != g.device:
            raise ValueError(f"{name} is on {p.device}, g on {g.device}")
    if len({p.data_ptr() for p, _ in state} | {g.data_ptr()}) != len(state) + 1:
        raise ValueError("clip_adam: w, m, v" + (", shadow" if ema is not None else "") + " and g must be distinct buffers")
    if g.numel() < 1:
        raise ValueError("clip_adam of an empty tensor")
    sumsq = _opt_f32(sumsq, "sumsq")
    if sumsq is not None and (sumsq.numel() != 1 or sumsq.device != g.device):
        raise ValueError(f"sumsq must be one float32 on {g.device}")
    lib, (w, m, v) = _lib.load(), [p for p, _ in state[:3]]
    if ema is None:
        check(lib.nd_clip_adam(ptr(w), ptr(m), ptr(v), ptr(g), g.numel(), ptr(sumsq), float(max_norm), ctypes.byref(adam), _stream(g)),
              "nd_clip_adam")
    else:
        check(lib.nd_clip_adam_ema(ptr(w), ptr(m), ptr(v), ptr(g), ptr(state[3][0]), g.numel(), ptr(sumsq), float(max_norm),
                                   ctypes.byref(adam), ctypes.byref(ema), _stream(g)), "nd_clip_adam_ema")
