"""What every wrapper module shares: the argument checks, the stream lookup, the per-stream workspace and the output containers' return.
Binds no entry point itself."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from .. import _lib
from .._lib import ND_ACT_GELU, ND_ACT_NONE, ND_ACT_RELU, ND_ACT_SOFTPLUS

ACT = {"none": ND_ACT_NONE, None: ND_ACT_NONE, "softplus": ND_ACT_SOFTPLUS, "relu": ND_ACT_RELU, "gelu": ND_ACT_GELU}


def _f32(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise _lib.NdError(f"{name} must be a GPU tensor (no CPU fallback)")
    if t.dtype != torch.float32:
        raise _lib.NdError(f"{name} must be float32")
    return t.contiguous()


def _opt_f32(t: Optional[torch.Tensor], name: str) -> Optional[torch.Tensor]:
    return _f32(t, name) if t is not None else None


def _inplace(t: Optional[torch.Tensor], name: str, dtype=torch.float32, shape=None) -> Optional[torch.Tensor]:
    """A tensor the kernel writes in place: on the GPU, of `dtype` and `shape`, and contiguous (a copy would lose the writes)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.NdError(f"{name} must be a GPU tensor (no CPU fallback)")
    if t.dtype != dtype:
        raise _lib.NdError(f"{name} must be {dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous (it is written in place)")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} is {tuple(t.shape)}; expected {tuple(shape)}")
    return t


class _DeviceState:
    """A per-image state the control kernels write in place.  The subclass sets B and `fields`: the (name, dtype, shape) of every
    tensor a kernel takes from it, at its own B."""

    def check(self, B: int) -> None:
        """The state belongs to a batch of B rows, and every field is still what the kernels may write in place."""
        if B != self.B:
            raise ValueError(f"the batch has {B} rows, the state {self.B}")
        for name, dtype, shape in self.fields:
            _inplace(getattr(self, name), name, dtype, shape)


def _on(t: torch.Tensor, name: str, shape: tuple, device) -> None:
    """The shape-and-device refusal: `t` must have exactly `shape` and live on `device`."""
    if tuple(t.shape) != shape or t.device != device:
        raise ValueError(f"{name} is {tuple(t.shape)} on {t.device}; expected {list(shape)} on {device}")


def _i64(t: torch.Tensor, device) -> torch.Tensor:
    return t.to(device=device, dtype=torch.int64).contiguous()


def _labels(labels: torch.Tensor, device, B: int, C: Optional[int] = None, who: str = "labels", also=()) -> torch.Tensor:
    """The labels as contiguous int64 [B] on `device`; `also`: the other per-image tensors the wrapper refuses in the same words
    (`who`).  C given: labels outside [0, C) are refused -- that reads back, the only host synchronisation of a wrapper that asks for
    it, so a wrapper passes C only behind its check_labels."""
    labels = labels.to(device=device, dtype=torch.int64).contiguous()
    for t in (labels, *also):
        if tuple(t.shape) != (B,):
            raise ValueError(f"{who} must be [{B}]")
    if C is not None and B and (int(labels.min()) < 0 or int(labels.max()) >= C):
        raise ValueError(f"labels must lie in [0, {C})")
    return labels


def _index(index: torch.Tensor, B: int, device) -> torch.Tensor:
    index = _i64(index, device)
    if tuple(index.shape) != (B,):
        raise ValueError(f"index must be [{B}] (the global image index of each row)")
    return index


def _per_image(x: torch.Tensor) -> Tuple[int, int]:
    B = x.shape[0] if x.dim() else 0
    per = x.numel() // max(B, 1)
    if B < 1 or per % 4:
        raise ValueError(f"need at least one image and a multiple of 4 elements per image (shape {tuple(x.shape)})")
    return B, per


def _image4(x: torch.Tensor, name: str) -> Tuple[int, int, int, int]:
    if x.dim() != 4 or x.shape[0] < 1:
        raise ValueError(f"{name} must be [B, Cin, H, W] with at least one image (shape {tuple(x.shape)})")
    return tuple(x.shape)


def _u64(v: int) -> int:
    """A Philox seed as the ABI's uint64 key word."""
    return int(v) & 0xFFFFFFFFFFFFFFFF


def _u32(v: int) -> int:
    """A restart or first-image number as the ABI's uint32 key word."""
    return int(v) & 0xFFFFFFFF


def _stream(t: torch.Tensor):
    return _lib.current_stream_ptr(t.device)


_ws_cache = {}


def _workspace(nbytes: int, device) -> torch.Tensor:
    key = (str(device), _lib.current_stream_ptr(device))   # one per stream: streams may run concurrently
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _ws_cache[key] = ws
    return ws


def _image_or_tensor(out: Optional[torch.Tensor], osp, want_out: bool, want_split: bool):
    """What a wrapper with the want_out / want_split pair returns: the fp32 tensor, its frag32b3 image, or both."""
    if want_out and want_split:
        return out, osp
    return osp if want_split else out
