"""Weight packing and the weight-streaming Linear with its input gradient.  Binds csrc/nd_pack.hip, csrc/nd_linear.hip and nd_linear_bwd
of csrc/nd_mlp_grad.hip (include/nested_diffusion.h: "standalone operators" and "the gradient through the mapping MLPs")."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib
from .._lib import check, ptr
from ._base import ACT, _f32, _on, _opt_f32, _stream, _workspace


class PackedWeight:
    """An nn.Linear weight [N, K] repacked once into the fragment order the streaming kernels read.
    dtype 'f16': the fp16-operand image (half the bytes; K % 32 == 0) -- the fp16 mode, not the reference's arithmetic."""

    def __init__(self, weight: torch.Tensor, dtype="f32"):
        lib = _lib.load()
        weight = _f32(weight, "weight")
        self.N, self.K = weight.shape
        self.dtype = _lib.dtype_code(dtype)
        nbytes = lib.nd_packed_bytes(self.N, self.K, self.dtype)
        if nbytes == 0:
            raise _lib.NdError(f"cannot pack a [{self.N}, {self.K}] weight: K must be a positive multiple of "
                               f"{32 if self.dtype == _lib.ND_DTYPE_F16 else 16}")
        self.data = torch.empty(nbytes // 4, dtype=torch.float32, device=weight.device)
        check(lib.nd_pack_rows(ptr(weight), ptr(self.data), self.N, self.K, self.dtype, _stream(weight)), "nd_pack_rows")

    def unpack(self) -> torch.Tensor:
        """The row-major [N, K] weight back out of an fp32 image (nd_unpack_rows: the exact inverse of the packing, padding rows dropped)."""
        if self.dtype != _lib.ND_DTYPE_F32:
            raise _lib.NdError("unpack reads fp32 weight images only: an fp16 PackedWeight does not hold the fp32 weight")
        out = torch.empty(self.N, self.K, dtype=torch.float32, device=self.data.device)
        check(_lib.load().nd_unpack_rows(ptr(self.data), ptr(out), self.N, self.K, self.dtype, _stream(self.data)), "nd_unpack_rows")
        return out

    def zeros_like(self) -> "PackedWeight":
        """An image of the same shape and dtype, all zero (Adam's m and v)."""
        z = object.__new__(PackedWeight)
        z.N, z.K, z.dtype, z.data = self.N, self.K, self.dtype, torch.zeros_like(self.data)
        return z


def linear(x: torch.Tensor, weight, bias: Optional[torch.Tensor] = None, act=None,
           scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act(scale * (x @ weight.T) + bias) for small row counts (weight streamed once).
    nn.Linear + ReLU of mapping/models/mlp.py:25-28.  `weight` is a PackedWeight (packed once) or a
    plain [N, K] tensor (packed on the fly: tests / one-off calls)."""
    lib = _lib.load()
    x = _f32(x, "x")
    M, K = x.shape
    if not isinstance(weight, PackedWeight):
        if weight.dim() != 2 or weight.shape[1] != K:
            raise ValueError(f"weight is {tuple(weight.shape)}, x is {tuple(x.shape)}")
        weight = PackedWeight(weight)
    N = weight.N
    if weight.K != K:
        raise ValueError(f"weight is [{weight.N}, {weight.K}], x is {tuple(x.shape)}")
    bias, scale = _opt_f32(bias, "bias"), _opt_f32(scale, "scale")
    out = torch.empty(M, N, dtype=torch.float32, device=x.device)
    nbytes = lib.nd_linear_workspace_bytes(M, K, N, weight.dtype)
    ws = _workspace(nbytes, x.device)
    check(lib.nd_linear(ptr(x), ptr(weight.data), ptr(scale), ptr(bias), ptr(out), M, K, N, ACT[act], weight.dtype, ptr(ws),
                        ws.numel(), _stream(x)), "nd_linear")
    return out


LINEAR_BWD_MAX_M = 128                                     # ND_LINEAR_BWD_MAX_M: rows per nd_linear_bwd launch


def linear_grad_input(dy: torch.Tensor, weight: PackedWeight, gate: Optional[torch.Tensor] = None,
                      add: Optional[torch.Tensor] = None) -> torch.Tensor:
    """((dy @ W) * (gate > 0)) + add: the input gradient of linear(x, weight) given dy = dL/d(its output) [M, N], read from the weight's
    packed image in place (no transposed copy).  gate [M, K]: the forward's post-ReLU input of that Linear (ReLU'(0) = 0), or None;
    add [M, K]: a gradient that joins at the Linear's input, or None.  More than 128 rows run as chunks of 128 (a row's result does not
    depend on the rows beside it: the chunks are the bits of one launch)."""
    lib = _lib.load()
    if not isinstance(weight, PackedWeight):
        raise TypeError("weight must be a PackedWeight (the image the forward streams)")
    if weight.dtype != _lib.ND_DTYPE_F32:
        raise _lib.NdError("linear_grad_input reads fp32 weight images only: the input gradient runs in fp32 mode, not on an fp16 PackedWeight")
    dy = _f32(dy, "dy")
    if dy.dim() != 2 or dy.shape[0] < 1 or dy.shape[1] != weight.N:
        raise ValueError(f"dy is {tuple(dy.shape)}, weight is [{weight.N}, {weight.K}]: expected [M >= 1, {weight.N}]")
    M, N, K = dy.shape[0], weight.N, weight.K
    if K % 16:
        raise ValueError(f"K must be a multiple of 16 (K={K})")
    gate, add = _opt_f32(gate, "gate"), _opt_f32(add, "add")
    for t, name in ((gate, "gate"), (add, "add")):
        if t is not None:
            _on(t, name, (M, K), dy.device)
    if weight.data.device != dy.device:
        raise ValueError(f"weight is on {weight.data.device}, dy on {dy.device}")
    out = torch.empty(M, K, dtype=torch.float32, device=dy.device)
    for s in range(0, M, LINEAR_BWD_MAX_M):
        e = min(s + LINEAR_BWD_MAX_M, M)
        check(lib.nd_linear_bwd(ptr(dy[s:e]), ptr(weight.data), ptr(gate[s:e]) if gate is not None else None,
                                ptr(add[s:e]) if add is not None else None, ptr(out[s:e]), e - s, N, K, weight.dtype, _stream(dy)),
              "nd_linear_bwd")
    return out
