"""The forward pieces of the ViT.  Binds csrc/nd_layernorm.hip, csrc/nd_attention.hip (with csrc/nd_attention_b9.hip), csrc/nd_patchify.hip
and the qkv-image entry points of csrc/nd_gemm_b9.hip (include/nested_diffusion.h: "standalone operators").  Each operator comes as a
pair: the fp32 result, or (`*_split`) the same result written as the frag32b3 image the gemm_split after it reads."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib
from .._lib import check, ptr
from ._base import _f32, _opt_f32, _stream
from .gemm import SplitMatrix


def _layernorm_args(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor):
    x = _f32(x, "x")
    dim = x.shape[-1]
    return x, _f32(weight, "weight"), _f32(bias, "bias"), x.numel() // dim, dim


def layernorm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float) -> torch.Tensor:
    x, weight, bias, rows, dim = _layernorm_args(x, weight, bias)
    out = torch.empty_like(x)
    check(_lib.load().nd_layernorm(ptr(x), ptr(weight), ptr(bias), ptr(out), rows, dim, float(eps), _stream(x)), "nd_layernorm")
    return out


def layernorm_split(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float) -> SplitMatrix:
    """LayerNorm with its result written as a frag32b3 image (the input of the gemm_split that follows it in a ViT block)."""
    x, weight, bias, rows, dim = _layernorm_args(x, weight, bias)
    out = SplitMatrix(rows, dim, x.device)
    check(_lib.load().nd_layernorm_split(ptr(x), ptr(weight), ptr(bias), ptr(out.data), rows, dim, float(eps), _stream(x)),
          "nd_layernorm_split")
    return out


def _attention_args(qkv: torch.Tensor, B: int, N: int, heads: int):
    qkv = _f32(qkv, "qkv")
    d = qkv.shape[-1] // (3 * heads)
    if qkv.numel() != B * N * 3 * heads * d:
        raise ValueError("qkv has the wrong number of elements")
    return qkv, d


def attention(qkv: torch.Tensor, B: int, N: int, heads: int, dtype="f32") -> torch.Tensor:
    """qkv: [B*N, 3*heads*64] (output of the qkv Linear) -> [B*N, heads*64].  dtype 'f16': fp16-operand contractions."""
    qkv, d = _attention_args(qkv, B, N, heads)
    out = torch.empty(B * N, heads * d, dtype=torch.float32, device=qkv.device)
    check(_lib.load().nd_attention(ptr(qkv), ptr(out), B, N, heads, d, _lib.dtype_code(dtype), _stream(qkv)), "nd_attention")
    return out


def attention_split(qkv: torch.Tensor, B: int, N: int, heads: int) -> SplitMatrix:
    """fp32 attention with its [B*N, heads*64] result written as a frag32b3 image (the input of the proj gemm_split)."""
    qkv, d = _attention_args(qkv, B, N, heads)
    out = SplitMatrix(B * N, heads * d, qkv.device)
    check(_lib.load().nd_attention_split(ptr(qkv), ptr(out.data), B, N, heads, d, _stream(qkv)), "nd_attention_split")
    return out


def qkv_images_supported(N: int, heads: int) -> bool:
    return bool(_lib.load().nd_qkv_images_supported(int(N), int(heads)))


def gemm_split_qkv(x: SplitMatrix, weight: SplitMatrix, bias: Optional[torch.Tensor], B: int, N: int, heads: int,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The qkv Linear of a ViT block (x: image of [B*N, K], weight: image of [3*heads*64, K]) with its result written as the attention's
    operand images (per image and head: q, k as frag32b3 blocks, v transposed; csrc/nd_b9.hpp).  Returns the opaque image buffer.
    out: an existing uint8 buffer of nd_qkv_images_bytes(B, N, heads) bytes to write into (rows / keys past N are never written:
    whatever it held stays there)."""
    lib = _lib.load()
    if x.rows != B * N or weight.rows != 3 * heads * 64 or weight.K != x.K:
        raise ValueError(f"x is {x.shape}, weight {weight.shape}: expected [{B * N}, K] and [{3 * heads * 64}, K]")
    nbytes = lib.nd_qkv_images_bytes(B, N, heads)
    if out is None:
        img = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    else:
        if out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous() or out.numel() != nbytes or out.device != x.device:
            raise ValueError(f"out must be a contiguous uint8 GPU buffer of {nbytes} bytes on {x.device}")
        img = out
    check(lib.nd_gemm_split_qkv(ptr(x.data), ptr(weight.data), ptr(_opt_f32(bias, "bias")), ptr(img), B, N, heads, x.K, _stream(x.data)),
          "nd_gemm_split_qkv")
    return img


def attention_images(img: torch.Tensor, B: int, N: int, heads: int, want_split: bool = False):
    """softmax(q k^T / 8) v on the bf16 matrix pipe with exact fp32 products, from the images gemm_split_qkv wrote: fp32 [B*N, heads*64], or
    (want_split) its frag32b3 image for the proj gemm_split."""
    out = SplitMatrix(B * N, heads * 64, img.device) if want_split else torch.empty(B * N, heads * 64, dtype=torch.float32, device=img.device)
    check(_lib.load().nd_attention_images(ptr(img), ptr(out.data if want_split else out), 1 if want_split else 0, B, N, heads, _stream(img)),
          "nd_attention_images")
    return out


def _patchify_args(img: torch.Tensor, p: int):
    """(img, its [B, Cin, H, W], the rows and columns of its im2col matrix)."""
    img = _f32(img, "img")
    B, Cin, H, W = img.shape
    return img, (B, Cin, H, W), B * (H // p) * (W // p), Cin * p * p


def patchify(img: torch.Tensor, p: int) -> torch.Tensor:
    """[B, Cin, H, W] -> [B*(H/p)*(W/p), Cin*p*p] (im2col for Conv2d(k=p, s=p))."""
    img, dims, rows, cols = _patchify_args(img, p)
    out = torch.empty(rows, cols, dtype=torch.float32, device=img.device)
    check(_lib.load().nd_patchify(ptr(img), ptr(out), *dims, p, _stream(img)), "nd_patchify")
    return out


def patchify_split(img: torch.Tensor, p: int) -> SplitMatrix:
    """im2col written as the frag32b3 image of [B*(H/p)*(W/p), Cin*p*p] (the input of the patch-embedding gemm_split)."""
    img, dims, rows, cols = _patchify_args(img, p)
    out = SplitMatrix(rows, cols, img.device)
    check(_lib.load().nd_patchify_split(ptr(img), ptr(out.data), *dims, p, _stream(img)), "nd_patchify_split")
    return out
