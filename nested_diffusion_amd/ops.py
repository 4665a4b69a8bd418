"""Thin torch-tensor wrappers over the standalone operators of libnd_hip.so.
Every function launches HIP kernels on torch's current stream; inputs must live on the GPU."""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import ND_ACT_GELU, ND_ACT_NONE, ND_ACT_RELU, ND_ACT_SOFTPLUS, check, ptr

ACT = {"none": ND_ACT_NONE, None: ND_ACT_NONE, "softplus": ND_ACT_SOFTPLUS, "relu": ND_ACT_RELU, "gelu": ND_ACT_GELU}


def _f32(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise _lib.NdError(f"{name} must be a GPU tensor (no CPU fallback)")
    if t.dtype != torch.float32:
        raise _lib.NdError(f"{name} must be float32")
    return t.contiguous()


def _stream(t: torch.Tensor):
    return torch.cuda.current_stream(t.device).cuda_stream


_ws_cache = {}


def _workspace(nbytes: int, device) -> torch.Tensor:
    key = (str(device), torch.cuda.current_stream(device).cuda_stream)   # one per stream: streams may run concurrently
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _ws_cache[key] = ws
    return ws


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
    wdata = weight.data
    bias = _f32(bias, "bias") if bias is not None else None
    scale = _f32(scale, "scale") if scale is not None else None
    out = torch.empty(M, N, dtype=torch.float32, device=x.device)
    nbytes = lib.nd_linear_workspace_bytes(M, K, N, weight.dtype)
    ws = _workspace(nbytes, x.device)
    check(lib.nd_linear(ptr(x), ptr(wdata), ptr(scale), ptr(bias), ptr(out), M, K, N, ACT[act], weight.dtype, ptr(ws),
                        ws.numel(), _stream(x)), "nd_linear")
    return out


class SplitMatrix:
    """frag32b3 image of an fp32 [rows, K] matrix (csrc/nd_b9.hpp): every value as its three exact bf16 pieces, in the lane order of
    v_mfma_f32_16x16x32_bf16 -- the operand form of nd_gemm_split.  Weights are converted once (at load); activations are written in
    this form by the operator that produces them."""

    def __init__(self, rows: int, K: int, device, data: Optional[torch.Tensor] = None):
        nbytes = _lib.load().nd_split_bytes(int(rows), int(K))
        if nbytes == 0:
            raise ValueError(f"no frag32b3 image for a [{rows}, {K}] matrix (K must be a positive multiple of 32)")
        self.rows, self.K = int(rows), int(K)
        self.data = data if data is not None else torch.empty(nbytes, dtype=torch.uint8, device=device)
        if self.data.numel() < nbytes or not self.data.is_cuda:
            raise ValueError("image buffer too small or not on the GPU")

    @property
    def shape(self):
        return (self.rows, self.K)

    @property
    def device(self):
        return self.data.device


def split_rows(x: torch.Tensor, out: Optional[SplitMatrix] = None) -> SplitMatrix:
    """fp32 [rows, K] -> its frag32b3 image (exact)."""
    x = _f32(x, "x")
    rows, K = x.shape
    out = out if out is not None else SplitMatrix(rows, K, x.device)
    check(_lib.load().nd_split_rows(ptr(x), ptr(out.data), rows, K, _stream(x)), "nd_split_rows")
    return out


def join_rows(s: SplitMatrix) -> torch.Tensor:
    """frag32b3 image -> fp32 [rows, K] (the three pieces summed: exact)."""
    out = torch.empty(s.rows, s.K, dtype=torch.float32, device=s.device)
    check(_lib.load().nd_join_rows(ptr(s.data), ptr(out), s.rows, s.K, _stream(out)), "nd_join_rows")
    return out


def gemm_split(x, weight: SplitMatrix, bias: Optional[torch.Tensor] = None, act=None, residual: Optional[torch.Tensor] = None,
               want_out: bool = True, want_split: bool = False, use_workspace: bool = True):
    """act(x @ weight.T + bias) + residual with exact fp32 products on the bf16 matrix pipe (nd_gemm_split).  x: fp32 [M, K] (split
    here) or a SplitMatrix.  Returns the fp32 result, its frag32b3 image (want_split; N % 32 == 0), or both as a tuple."""
    lib = _lib.load()
    xs = x if isinstance(x, SplitMatrix) else split_rows(x)
    M, K = xs.shape
    N = weight.rows
    if weight.K != K:
        raise ValueError(f"weight is {weight.shape}, x is {xs.shape}")
    dev = xs.device
    bias = _f32(bias, "bias") if bias is not None else None
    residual = _f32(residual, "residual") if residual is not None else None
    if residual is not None and tuple(residual.shape) != (M, N):
        raise ValueError("residual must be [M, N]")
    out = torch.empty(M, N, dtype=torch.float32, device=dev) if want_out else None
    osp = SplitMatrix(M, N, dev) if want_split else None
    nbytes = lib.nd_gemm_split_workspace_bytes(M, K, N) if use_workspace else 0
    ws = _workspace(nbytes, dev) if nbytes else None
    check(lib.nd_gemm_split(ptr(xs.data), ptr(weight.data), ptr(bias), ptr(residual), ptr(out), ptr(osp.data) if osp else None, M, K, N,
                            ACT[act], ptr(ws), ws.numel() if ws is not None else 0, _stream(xs.data)), "nd_gemm_split")
    if want_out and want_split:
        return out, osp
    return osp if want_split else out


def gemm_bias_act(x: torch.Tensor, weight, bias: Optional[torch.Tensor] = None, act=None,
                  residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act(x @ weight.T + bias) + residual for large row counts (ViT token matrices).  The kernel follows the WEIGHT the caller holds:
    a SplitMatrix (frag32b3 image made once with split_rows, as mapping.VisionTransformer does): exact fp32 products on the bf16
    matrix pipe (gemm_split); a plain fp32 tensor: the f32-input-MFMA kernel (any K % 16 == 0) -- never an implicit re-split of the
    whole weight per call; a float16 tensor: the fp16-operand kernel (x rounded to fp16 on the fly, fp32 accumulate / out; K % 32 == 0)."""
    lib = _lib.load()
    if isinstance(weight, SplitMatrix):
        return gemm_split(x, weight, bias, act, residual)
    x = _f32(x, "x")
    if not weight.is_cuda:
        raise _lib.NdError("weight must be a GPU tensor (no CPU fallback)")
    if weight.dtype == torch.float16:
        weight, dt = weight.contiguous(), _lib.ND_DTYPE_F16
    else:
        weight, dt = _f32(weight, "weight"), _lib.ND_DTYPE_F32
    M, K = x.shape
    N = weight.shape[0]
    if weight.shape[1] != K:
        raise ValueError(f"weight is {tuple(weight.shape)}, x is {tuple(x.shape)}")
    bias = _f32(bias, "bias") if bias is not None else None
    residual = _f32(residual, "residual") if residual is not None else None
    if residual is not None and tuple(residual.shape) != (M, N):
        raise ValueError("residual must be [M, N]")
    out = torch.empty(M, N, dtype=torch.float32, device=x.device)
    nbytes = lib.nd_gemm_workspace_bytes(M, K, N, dt)
    ws = _workspace(nbytes, x.device) if nbytes else None
    check(lib.nd_gemm_bias_act(ptr(x), ptr(weight), ptr(bias), ptr(residual), ptr(out), M, K, N, ACT[act], dt, ptr(ws),
                               ws.numel() if ws is not None else 0, _stream(x)), "nd_gemm_bias_act")
    return out


def layernorm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float) -> torch.Tensor:
    lib = _lib.load()
    x = _f32(x, "x")
    dim = x.shape[-1]
    rows = x.numel() // dim
    out = torch.empty_like(x)
    check(lib.nd_layernorm(ptr(x), ptr(_f32(weight, "weight")), ptr(_f32(bias, "bias")), ptr(out), rows, dim, float(eps),
                           _stream(x)), "nd_layernorm")
    return out


def layernorm_split(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float) -> SplitMatrix:
    """LayerNorm with its result written as a frag32b3 image (the input of the gemm_split that follows it in a ViT block)."""
    x = _f32(x, "x")
    dim = x.shape[-1]
    rows = x.numel() // dim
    out = SplitMatrix(rows, dim, x.device)
    check(_lib.load().nd_layernorm_split(ptr(x), ptr(_f32(weight, "weight")), ptr(_f32(bias, "bias")), ptr(out.data), rows, dim, float(eps),
                                         _stream(x)), "nd_layernorm_split")
    return out


def attention_split(qkv: torch.Tensor, B: int, N: int, heads: int) -> SplitMatrix:
    """fp32 attention with its [B*N, heads*64] result written as a frag32b3 image (the input of the proj gemm_split)."""
    qkv = _f32(qkv, "qkv")
    d = qkv.shape[-1] // (3 * heads)
    if qkv.numel() != B * N * 3 * heads * d:
        raise ValueError("qkv has the wrong number of elements")
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
    check(lib.nd_gemm_split_qkv(ptr(x.data), ptr(weight.data), ptr(_f32(bias, "bias")) if bias is not None else None, ptr(img), B, N, heads, x.K,
                                _stream(x.data)), "nd_gemm_split_qkv")
    return img


def attention_images(img: torch.Tensor, B: int, N: int, heads: int, want_split: bool = False):
    """softmax(q k^T / 8) v on the bf16 matrix pipe with exact fp32 products, from the images gemm_split_qkv wrote: fp32 [B*N, heads*64], or
    (want_split) its frag32b3 image for the proj gemm_split."""
    out = SplitMatrix(B * N, heads * 64, img.device) if want_split else torch.empty(B * N, heads * 64, dtype=torch.float32, device=img.device)
    check(_lib.load().nd_attention_images(ptr(img), ptr(out.data if want_split else out), 1 if want_split else 0, B, N, heads, _stream(img)),
          "nd_attention_images")
    return out


def patchify_split(img: torch.Tensor, p: int) -> SplitMatrix:
    """im2col written as the frag32b3 image of [B*(H/p)*(W/p), Cin*p*p] (the input of the patch-embedding gemm_split)."""
    img = _f32(img, "img")
    B, Cin, H, W = img.shape
    out = SplitMatrix(B * (H // p) * (W // p), Cin * p * p, img.device)
    check(_lib.load().nd_patchify_split(ptr(img), ptr(out.data), B, Cin, H, W, p, _stream(img)), "nd_patchify_split")
    return out


def attention(qkv: torch.Tensor, B: int, N: int, heads: int, dtype="f32") -> torch.Tensor:
    """qkv: [B*N, 3*heads*64] (output of the qkv Linear) -> [B*N, heads*64].  dtype 'f16': fp16-operand contractions."""
    lib = _lib.load()
    qkv = _f32(qkv, "qkv")
    d = qkv.shape[-1] // (3 * heads)
    if qkv.numel() != B * N * 3 * heads * d:
        raise ValueError("qkv has the wrong number of elements")
    out = torch.empty(B * N, heads * d, dtype=torch.float32, device=qkv.device)
    check(lib.nd_attention(ptr(qkv), ptr(out), B, N, heads, d, _lib.dtype_code(dtype), _stream(qkv)), "nd_attention")
    return out


def patchify(img: torch.Tensor, p: int) -> torch.Tensor:
    """[B, Cin, H, W] -> [B*(H/p)*(W/p), Cin*p*p] (im2col for Conv2d(k=p, s=p))."""
    lib = _lib.load()
    img = _f32(img, "img")
    B, Cin, H, W = img.shape
    out = torch.empty(B * (H // p) * (W // p), Cin * p * p, dtype=torch.float32, device=img.device)
    check(lib.nd_patchify(ptr(img), ptr(out), B, Cin, H, W, p, _stream(img)), "nd_patchify")
    return out


def softmax_rows(x: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    x = _f32(x, "x")
    C = x.shape[-1]
    out = torch.empty_like(x)
    check(lib.nd_softmax_rows(ptr(x), ptr(out), x.numel() // C, C, _stream(x)), "nd_softmax_rows")
    return out


def aggregate(samples: torch.Tensor, temperature: float, return_probs: bool = False
              ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """samples [S, B, C] -> (prob [B, C], vote [B] int64, per-sample probs [S, B, C] or None).
    convert_to_prob + compute_ensemble_confidence + majority_voting_for_mc_samples
    (classification_train_separately.py:392-398, 425-447, 51-68)."""
    lib = _lib.load()
    samples = _f32(samples, "samples")
    S, B, C = samples.shape
    prob = torch.empty(B, C, dtype=torch.float32, device=samples.device)
    vote = torch.empty(B, dtype=torch.int64, device=samples.device)
    probs = torch.empty_like(samples) if return_probs else None
    check(lib.nd_aggregate(ptr(samples), ptr(prob), ptr(vote), ptr(probs), S, B, C, float(temperature), _stream(samples)),
          "nd_aggregate")
    return prob, vote, probs


def sample_stats(probs: torch.Tensor, q_lo: float = 0.025, q_hi: float = 0.975) -> Tuple[torch.Tensor, torch.Tensor]:
    """probs [S, B, C] -> (PIW [B, C] = quantile(q_hi) - quantile(q_lo) over S, unbiased variance [B, C]).
    compute_mean_piws_for_class :108-114, calculate_variances :166-172."""
    lib = _lib.load()
    probs = _f32(probs, "probs")
    S, B, C = probs.shape
    piw = torch.empty(B, C, dtype=torch.float32, device=probs.device)
    var = torch.empty(B, C, dtype=torch.float32, device=probs.device)
    check(lib.nd_sample_stats(ptr(probs), ptr(piw), ptr(var), S, B, C, float(q_lo), float(q_hi), _stream(probs)), "nd_sample_stats")
    return piw, var


def report(piw: torch.Tensor, var: torch.Tensor, prob_mean: torch.Tensor, vote: torch.Tensor, target: torch.Tensor,
           temperature: float, n_bins: int = 10) -> dict:
    """The numbers test_atk prints (classification_train_separately.py:801-838)."""
    lib = _lib.load()
    piw, var, prob_mean = _f32(piw, "piw"), _f32(var, "var"), _f32(prob_mean, "prob_mean")
    N, C = prob_mean.shape
    vote = vote.to(device=piw.device, dtype=torch.int64).contiguous()
    target = target.to(device=piw.device, dtype=torch.int64).contiguous()
    out = torch.empty(2 + 4 * C, dtype=torch.float32, device=piw.device)
    check(lib.nd_report(ptr(piw), ptr(var), ptr(prob_mean), ptr(vote), ptr(target), ptr(out), N, C, float(temperature), int(n_bins),
                        _stream(piw)), "nd_report")
    o = out.cpu()
    return {"accuracy": o[0], "ece": o[1], "piw_correct": o[2:2 + C], "piw_incorrect": o[2 + C:2 + 2 * C],
            "var_correct": o[2 + 2 * C:2 + 3 * C], "var_incorrect": o[2 + 3 * C:2 + 4 * C]}


# ---- input gradient of the ViT (csrc/nd_vit_grad.hip) and the Linf attack steps (csrc/nd_attack_linf.hip) ---------------------
def _image_or_tensor(out: torch.Tensor, osp: Optional[SplitMatrix], want_out: bool, want_split: bool):
    if want_out and want_split:
        return out, osp
    return osp if want_split else out


def layernorm_grad(x: torch.Tensor, weight: torch.Tensor, g: torch.Tensor, eps: float, residual: Optional[torch.Tensor] = None,
                   want_out: bool = True, want_split: bool = False):
    """Input gradient of LayerNorm(x) * weight + bias given g = dL/d(output), plus `residual` (the gradient the residual stream carries
    past the LayerNorm).  mean / rstd are recomputed from x.  Returns fp32 [rows, dim], its frag32b3 image (want_split), or both."""
    x, g = _f32(x, "x"), _f32(g, "g")
    if g.shape != x.shape:
        raise ValueError(f"g is {tuple(g.shape)}, x is {tuple(x.shape)}")
    residual = _f32(residual, "residual") if residual is not None else None
    if residual is not None and residual.shape != x.shape:
        raise ValueError("residual must have the shape of x")
    if not (want_out or want_split):
        raise ValueError("nothing to return")
    dim = x.shape[-1]
    rows = x.numel() // dim
    out = torch.empty_like(x) if want_out else None
    osp = SplitMatrix(rows, dim, x.device) if want_split else None
    check(_lib.load().nd_layernorm_bwd(ptr(x), ptr(_f32(weight, "weight")), ptr(g), ptr(residual), ptr(out), ptr(osp.data) if osp else None,
                                       rows, dim, float(eps), _stream(x)), "nd_layernorm_bwd")
    return _image_or_tensor(out, osp, want_out, want_split)


def gelu_split(u: torch.Tensor, want_out: bool = False):
    """GELU(u) (exact erf, the expression of the fc1 epilogue) written as the frag32b3 image of [rows, cols] (and fp32 with want_out)."""
    u = _f32(u, "u")
    rows, cols = u.shape
    out = torch.empty_like(u) if want_out else None
    osp = SplitMatrix(rows, cols, u.device)
    check(_lib.load().nd_gelu_split(ptr(u), ptr(out), ptr(osp.data), rows, cols, _stream(u)), "nd_gelu_split")
    return _image_or_tensor(out, osp, want_out, True)


def gelu_grad_split(u: torch.Tensor, dg: torch.Tensor, want_out: bool = False):
    """dg * GELU'(u) as the frag32b3 image of [rows, cols] (and fp32 with want_out)."""
    u, dg = _f32(u, "u"), _f32(dg, "dg")
    if dg.shape != u.shape:
        raise ValueError(f"dg is {tuple(dg.shape)}, u is {tuple(u.shape)}")
    rows, cols = u.shape
    out = torch.empty_like(u) if want_out else None
    osp = SplitMatrix(rows, cols, u.device)
    check(_lib.load().nd_gelu_bwd_split(ptr(u), ptr(dg), ptr(out), ptr(osp.data), rows, cols, _stream(u)), "nd_gelu_bwd_split")
    return _image_or_tensor(out, osp, want_out, True)


ATTENTION_BWD_MAX_TOKENS = 208      # ATB_NMAX of csrc/nd_vit_grad.hip: the keys per (image, head) k_attention_bwd holds in LDS


def attention_grad(qkv: torch.Tensor, o: torch.Tensor, dout: torch.Tensor, B: int, N: int, heads: int, want_out: bool = True,
                   want_split: bool = False):
    """dqkv [B*N, 3*heads*64] of o = softmax(q k^T / 8) v (timm layout) given dout = dL/do; fp32, its frag32b3 image, or both."""
    qkv, o, dout = _f32(qkv, "qkv"), _f32(o, "o"), _f32(dout, "dout")
    if tuple(qkv.shape) != (B * N, 3 * heads * 64) or tuple(o.shape) != (B * N, heads * 64) or dout.shape != o.shape:
        raise ValueError(f"qkv {tuple(qkv.shape)}, o {tuple(o.shape)}, dout {tuple(dout.shape)} do not match B={B}, N={N}, heads={heads}")
    if not (want_out or want_split):
        raise ValueError("nothing to return")
    out = torch.empty_like(qkv) if want_out else None
    osp = SplitMatrix(B * N, 3 * heads * 64, qkv.device) if want_split else None
    check(_lib.load().nd_attention_bwd(ptr(qkv), ptr(o), ptr(dout), ptr(out), ptr(osp.data) if osp else None, B, N, heads, _stream(qkv)),
          "nd_attention_bwd")
    return _image_or_tensor(out, osp, want_out, want_split)


def xent_head_grad(logits: torch.Tensor, labels: torch.Tensor, head_w: torch.Tensor,
                   check_labels: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dfeat [B, E] = (softmax(logits) - onehot(labels)) . head_w, per-image cross-entropy [B]): the gradient of
    crossentropy(logits, labels).sum() with respect to the head's input.  check_labels=False skips the label-range check, the call's only
    read-back."""
    logits, head_w = _f32(logits, "logits"), _f32(head_w, "head_w")
    B, C = logits.shape
    if head_w.dim() != 2 or head_w.shape[0] != C:
        raise ValueError(f"head_w is {tuple(head_w.shape)}, logits {tuple(logits.shape)}")
    labels = labels.to(device=logits.device, dtype=torch.int64).contiguous()
    if labels.shape != (B,):
        raise ValueError(f"labels must be [{B}]")
    if check_labels and B and (int(labels.min()) < 0 or int(labels.max()) >= C):
        raise ValueError(f"labels must lie in [0, {C})")
    E = head_w.shape[1]
    dfeat = torch.empty(B, E, dtype=torch.float32, device=logits.device)
    loss = torch.empty(B, dtype=torch.float32, device=logits.device)
    check(_lib.load().nd_xent_head_bwd(ptr(logits), ptr(labels), ptr(head_w), ptr(dfeat), ptr(loss), B, C, E, _stream(logits)),
          "nd_xent_head_bwd")
    return dfeat, loss


def unpatchify(cols: torch.Tensor, B: int, Cin: int, H: int, W: int, p: int) -> torch.Tensor:
    """[B*(H/p)*(W/p), Cin*p*p] -> [B, Cin, H, W]: the exact inverse of patchify."""
    cols = _f32(cols, "cols")
    if H % p or W % p or tuple(cols.shape) != (B * (H // p) * (W // p), Cin * p * p):
        raise ValueError(f"cols is {tuple(cols.shape)}; expected [{B * (H // p) * (W // p)}, {Cin * p * p}]")
    img = torch.empty(B, Cin, H, W, dtype=torch.float32, device=cols.device)
    check(_lib.load().nd_unpatchify(ptr(cols), ptr(img), B, Cin, H, W, p, _stream(cols)), "nd_unpatchify")
    return img


def linf_step(x: torch.Tensor, x0: torch.Tensor, grad: Optional[torch.Tensor], alpha: float, eps: float, lo: float = 0.0,
              hi: float = 1.0) -> torch.Tensor:
    """clip(x0 + clip(x + alpha * sign(grad) - x0, -eps, eps), lo, hi) (foolbox's step, project, clip).  grad None: no step --
    with lo = -inf, hi = inf that is foolbox's final clip_perturbation."""
    x, x0 = _f32(x, "x"), _f32(x0, "x0")
    if x0.shape != x.shape:
        raise ValueError("x0 must have the shape of x")
    if grad is not None:
        grad = _f32(grad, "grad")
        if grad.shape != x.shape:
            raise ValueError("grad must have the shape of x")
    out = torch.empty_like(x)
    check(_lib.load().nd_linf_step(ptr(x), ptr(x0), ptr(grad), ptr(out), x.numel(), float(alpha), float(eps), float(lo), float(hi),
                                   _stream(x)), "nd_linf_step")
    return out


def linf_random_start(x0: torch.Tensor, eps: float, seed: int, first_image: int = 0, restart: int = 0, lo: float = 0.0,
                      hi: float = 1.0) -> torch.Tensor:
    """clip(x0 + U[-eps, eps), lo, hi) per image; the draws of image b are keyed on (seed, first_image + b, element, restart), so an
    image draws the same start at any batch size (include/nested_diffusion.h: nd_linf_random_start)."""
    x0 = _f32(x0, "x0")
    B = x0.shape[0]
    per = x0.numel() // max(B, 1)
    if per % 4:
        raise ValueError("the elements per image must be a multiple of 4")
    out = torch.empty_like(x0)
    check(_lib.load().nd_linf_random_start(ptr(x0), ptr(out), B, per, int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_image) & 0xFFFFFFFF,
                                           int(restart) & 0xFFFFFFFF, float(eps), float(lo), float(hi), _stream(x0)), "nd_linf_random_start")
    return out


# ---- AutoAttack APGD-CE, Linf (include/nested_diffusion.h: nd_apgd_*; the loop: autoattack.py) ----------------------------------------
APGD_NOT_PRED, APGD_IMPROVED, APGD_RESTORE = 1, 2, 4       # ND_APGD_* flag bits


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


def _per_image(x: torch.Tensor) -> Tuple[int, int]:
    B = x.shape[0] if x.dim() else 0
    per = x.numel() // max(B, 1)
    if B < 1 or per % 4:
        raise ValueError(f"need at least one image and a multiple of 4 elements per image (shape {tuple(x.shape)})")
    return B, per


def apgd_random_start(x0: torch.Tensor, index: torch.Tensor, eps: float, seed: int, restart: int = 0, lo: float = 0.0,
                      hi: float = 1.0) -> torch.Tensor:
    """APGD's start clip(x0 + eps * t / (max|t| + 1e-12), lo, hi), t = 2 U[0, 1) - 1 per element, max per image; row b draws with the key
    (seed, index[b], element, restart), so a row of a compacted subset draws what it draws in the full batch."""
    x0 = _f32(x0, "x0")
    B, per = _per_image(x0)
    index = _index(index, B, x0.device)
    out = torch.empty_like(x0)
    m_ws = torch.empty(B, dtype=torch.int32, device=x0.device)
    check(_lib.load().nd_apgd_random_start(ptr(x0), ptr(index), ptr(out), ptr(m_ws), B, per, int(seed) & 0xFFFFFFFFFFFFFFFF,
                                           int(restart) & 0xFFFFFFFF, float(eps), float(lo), float(hi), _stream(x0)), "nd_apgd_random_start")
    return out


class ApgdState:
    """APGD's per-image state on the device (nd_apgd_control): step, loss_best, loss_best_last_check (fp32 [B]), reduced_last_check, acc
    (int32 [B]), loss_steps (fp32 [n_iter, B]) and the flags of the last iteration (int32 [B])."""

    def __init__(self, B: int, n_iter: int, device):
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=device)     # noqa: E731
        i = lambda *s: torch.empty(*s, dtype=torch.int32, device=device)       # noqa: E731
        self.B, self.n_iter = B, n_iter
        self.step, self.loss_best, self.loss_best_last_check = f(B), f(B), f(B)
        self.reduced_last_check, self.acc, self.flags = i(B), i(B), i(B)
        self.loss_steps = f(n_iter, B)


def apgd_control(logits: torch.Tensor, labels: torch.Tensor, loss: torch.Tensor, state: ApgdState, it: int, k: int = 0, rho: float = 0.75,
                 step0: float = 0.0) -> torch.Tensor:
    """APGD's per-image bookkeeping of iteration `it` (-1: initialise from the start point, step = step0), with a checkpoint of length k
    when k > 0; updates `state` in place on the device and returns state.flags (APGD_NOT_PRED | APGD_IMPROVED | APGD_RESTORE).
    Nothing is read back to the host."""
    logits = _f32(logits, "logits")
    if logits.dim() != 2:
        raise ValueError("logits must be [B, C]")
    B, C = logits.shape
    if C < 1 or C > 1024:
        raise ValueError(f"apgd control takes 1 <= C <= 1024 classes (C={C})")
    if B != state.B:
        raise ValueError(f"logits has {B} rows, the state {state.B}")
    labels = labels.to(device=logits.device, dtype=torch.int64).contiguous()
    loss = _f32(loss, "loss")
    if tuple(labels.shape) != (B,) or tuple(loss.shape) != (B,):
        raise ValueError(f"labels and loss must be [{B}]")
    if not -1 <= it < state.n_iter or not 0 <= k <= it + 1:
        raise ValueError(f"need -1 <= it < n_iter and 0 <= k <= it + 1 (it={it}, k={k}, n_iter={state.n_iter})")
    s = state
    for name in ("step", "loss_best", "loss_best_last_check"):
        _inplace(getattr(s, name), name, torch.float32, (B,))
    for name in ("reduced_last_check", "acc", "flags"):
        _inplace(getattr(s, name), name, torch.int32, (B,))
    _inplace(s.loss_steps, "loss_steps", torch.float32, (s.n_iter, B))
    check(_lib.load().nd_apgd_control(ptr(logits), ptr(labels), ptr(loss), ptr(s.step), ptr(s.loss_best), ptr(s.loss_best_last_check),
                                      ptr(s.reduced_last_check), ptr(s.acc), ptr(s.loss_steps), ptr(s.flags), B, C, s.n_iter, int(it),
                                      int(k), float(rho), float(step0), _stream(logits)), "nd_apgd_control")
    return s.flags


def apgd_update(x: torch.Tensor, x_adv: torch.Tensor, x_adv_old: Optional[torch.Tensor], grad: torch.Tensor,
                x_best: Optional[torch.Tensor], grad_best: Optional[torch.Tensor], x_best_adv: Optional[torch.Tensor],
                flags: Optional[torch.Tensor], step: Optional[torch.Tensor], eps: float, a: float, do_step: bool) -> None:
    """APGD's per-element work of one iteration, in place: the flags' copies (x_best_adv, x_best / grad_best, the restore), then with
    do_step the momentum step of coefficient a from x_adv (or the restored x_best) to the next iterate (x_adv, x_adv_old).
    flags None: the step alone (the first step: a = 1, with x_adv_old a copy of x_adv)."""
    x_adv = _inplace(x_adv, "x_adv")
    B, per = _per_image(x_adv)
    shape = tuple(x_adv.shape)
    grad = _inplace(grad, "grad", shape=shape)
    if flags is not None:
        flags = _inplace(flags, "flags", torch.int32, (B,))
        if x_best is None or grad_best is None or x_best_adv is None:
            raise ValueError("the flags need x_best, grad_best and x_best_adv")
        x_best, grad_best, x_best_adv = (_inplace(t, n, shape=shape) for t, n in ((x_best, "x_best"), (grad_best, "grad_best"),
                                                                                   (x_best_adv, "x_best_adv")))
    if do_step:
        if x is None or x_adv_old is None or step is None:
            raise ValueError("a step needs x, x_adv_old and step")
        x, x_adv_old = _inplace(x, "x", shape=shape), _inplace(x_adv_old, "x_adv_old", shape=shape)
        step = _inplace(step, "step", shape=(B,))
    check(_lib.load().nd_apgd_update(ptr(x) if do_step else None, ptr(x_adv), ptr(x_adv_old) if do_step else None, ptr(grad),
                                     ptr(x_best), ptr(grad_best), ptr(x_best_adv), ptr(flags), ptr(step) if do_step else None, B, per,
                                     float(eps), float(a), int(bool(do_step)), _stream(x_adv)), "nd_apgd_update")


# ---- the Square attack, Linf (include/nested_diffusion.h: nd_square_*; the loop: square.py) --------------------------------------------
SQUARE_ACTIVE, SQUARE_ACCEPT = 1, 2                        # ND_SQUARE_* flag bits


def _image4(x: torch.Tensor, name: str) -> Tuple[int, int, int, int]:
    if x.dim() != 4 or x.shape[0] < 1:
        raise ValueError(f"{name} must be [B, Cin, H, W] with at least one image (shape {tuple(x.shape)})")
    return tuple(x.shape)


def _index(index: torch.Tensor, B: int, device) -> torch.Tensor:
    index = index.to(device=device, dtype=torch.int64).contiguous()
    if tuple(index.shape) != (B,):
        raise ValueError(f"index must be [{B}] (the global image index of each row)")
    return index


class SquareState:
    """The Square attack's per-image state on the device (nd_square_accept): margin_min, loss_min (fp32 [B]), n_queries and the flags of
    the last query (int32 [B]), and the window corner (vh, vw) of the last proposal (win, int32 [B, 2])."""

    def __init__(self, B: int, device):
        self.B = B
        self.margin_min = torch.empty(B, dtype=torch.float32, device=device)
        self.loss_min = torch.empty(B, dtype=torch.float32, device=device)
        self.n_queries = torch.empty(B, dtype=torch.int32, device=device)
        self.flags = torch.empty(B, dtype=torch.int32, device=device)
        self.win = torch.zeros(B, 2, dtype=torch.int32, device=device)


def square_init(x0: torch.Tensor, index: torch.Tensor, eps: float, seed: int, restart: int = 0, lo: float = 0.0,
                hi: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(x_best, x_new), both the vertical-stripe start clip(x0 + eps * sigma(b, c, w), lo, hi); row b draws its signs with the key
    (seed, index[b], c * W + w, restart), so a row of a compacted subset draws what it draws in the full batch."""
    x0 = _f32(x0, "x0")
    B, Cin, H, W = _image4(x0, "x0")
    index = _index(index, B, x0.device)
    x_best, x_new = torch.empty_like(x0), torch.empty_like(x0)
    check(_lib.load().nd_square_init(ptr(x0), ptr(index), ptr(x_best), ptr(x_new), B, Cin, H, W, int(seed) & 0xFFFFFFFFFFFFFFFF,
                                     int(restart) & 0xFFFFFFFF, float(eps), float(lo), float(hi), _stream(x0)), "nd_square_init")
    return x_best, x_new


def _square_state(state: SquareState, B: int) -> None:
    if B != state.B:
        raise ValueError(f"the batch has {B} rows, the state {state.B}")
    for name in ("margin_min", "loss_min"):
        _inplace(getattr(state, name), name, torch.float32, (B,))
    for name in ("n_queries", "flags"):
        _inplace(getattr(state, name), name, torch.int32, (B,))
    _inplace(state.win, "win", torch.int32, (B, 2))


def square_propose(x0: torch.Tensor, x_best: torch.Tensor, x_new: torch.Tensor, index: torch.Tensor, state: SquareState, s: int, it: int,
                   eps: float, seed: int, restart: int = 0, lo: float = 0.0, hi: float = 1.0) -> None:
    """Query `it` of the rows still active (state.margin_min > 0): draws each row's window and per-channel signs, writes the candidate
    clip(min(max(x_best +- 2 eps, x0 - eps), x0 + eps), lo, hi) into that window of x_new and the corner into state.win.  In place;
    frozen rows are not touched."""
    x_new = _inplace(x_new, "x_new")
    B, Cin, H, W = _image4(x_new, "x_new")
    shape = tuple(x_new.shape)
    x0, x_best = _inplace(x0, "x0", shape=shape), _inplace(x_best, "x_best", shape=shape)
    index = _index(index, B, x_new.device)
    _square_state(state, B)
    if not 1 <= s <= min(H, W) or it < 0:
        raise ValueError(f"need 1 <= s <= min(H, W) and it >= 0 (s={s}, H={H}, W={W}, it={it})")
    check(_lib.load().nd_square_propose(ptr(x0), ptr(x_best), ptr(x_new), ptr(index), ptr(state.margin_min), ptr(state.win), B, Cin, H, W,
                                        int(s), int(it), int(seed) & 0xFFFFFFFFFFFFFFFF, int(restart) & 0xFFFFFFFF, float(eps), float(lo),
                                        float(hi), _stream(x_new)), "nd_square_propose")


def square_accept(scores: torch.Tensor, labels: torch.Tensor, state: SquareState, it: int) -> torch.Tensor:
    """The bookkeeping of query `it` (-1: initialise from the start point's scores) on the device: the margin of each row, the accept rule,
    the query count; updates `state` in place and returns state.flags (SQUARE_ACTIVE | SQUARE_ACCEPT).  Nothing is read back."""
    scores = _f32(scores, "scores")
    if scores.dim() != 2:
        raise ValueError("scores must be [B, C]")
    B, C = scores.shape
    if C < 2 or C > 1024:
        raise ValueError(f"square accept takes 2 <= C <= 1024 classes (C={C})")
    labels = labels.to(device=scores.device, dtype=torch.int64).contiguous()
    if tuple(labels.shape) != (B,):
        raise ValueError(f"labels must be [{B}]")
    _square_state(state, B)
    if it < -1:
        raise ValueError(f"need it >= -1 (it={it})")
    check(_lib.load().nd_square_accept(ptr(scores), ptr(labels), ptr(state.margin_min), ptr(state.loss_min), ptr(state.n_queries),
                                       ptr(state.flags), B, C, int(it), _stream(scores)), "nd_square_accept")
    return state.flags


def square_commit(x_best: torch.Tensor, x_new: torch.Tensor, state: SquareState, s: int) -> None:
    """Over each active row's window (state.win, side s of the propose): an accepted candidate becomes x_best, a rejected one is
    restored from x_best.  Afterwards x_new == x_best everywhere."""
    x_new = _inplace(x_new, "x_new")
    B, Cin, H, W = _image4(x_new, "x_new")
    x_best = _inplace(x_best, "x_best", shape=tuple(x_new.shape))
    _square_state(state, B)
    if not 1 <= s <= min(H, W):
        raise ValueError(f"need 1 <= s <= min(H, W) (s={s}, H={H}, W={W})")
    check(_lib.load().nd_square_commit(ptr(x_best), ptr(x_new), ptr(state.win), ptr(state.flags), B, Cin, H, W, int(s), _stream(x_new)),
          "nd_square_commit")


# ---- the L2 attacks and Carlini & Wagner (include/nested_diffusion.h: nd_l2_*, nd_cw_*, nd_margin_head_bwd; the loops: attack.py) -----
L2_MAX_PARTS = 256                                         # ND_L2_MAX_PARTS: partials per image of a row reduction


def _l2_ws(B: int, device, sums: int = 2) -> torch.Tensor:
    """The row reductions' workspace: ND_L2_MAX_PARTS partials per image and sum (written before it is read: no initialisation)."""
    return torch.empty(sums * L2_MAX_PARTS * B, dtype=torch.float32, device=device)


def margin_head_grad(logits: torch.Tensor, labels: torch.Tensor, consts: torch.Tensor, head_w: torch.Tensor, confidence: float = 0.0,
                     check_labels: bool = True) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dfeat [B, E], margin [B], other [B] int32): the gradient of sum_b consts[b] * max(0, margin[b]) with respect to the head's input,
    margin = logits[label] - logits[other] + confidence, other = the first maximal non-label column (nd_margin_head_bwd).
    check_labels=False skips the label-range check, which reads back (the kernel gives an out-of-range label a NaN margin and no
    gradient): a loop that checked its labels once stays free of host synchronisation."""
    logits, head_w, consts = _f32(logits, "logits"), _f32(head_w, "head_w"), _f32(consts, "consts")
    if logits.dim() != 2:
        raise ValueError("logits must be [B, C]")
    B, C = logits.shape
    if C < 2 or C > 1024:
        raise ValueError(f"the margin needs 2 <= C <= 1024 classes (C={C})")
    if head_w.dim() != 2 or head_w.shape[0] != C:
        raise ValueError(f"head_w is {tuple(head_w.shape)}, logits {tuple(logits.shape)}")
    labels = labels.to(device=logits.device, dtype=torch.int64).contiguous()
    if tuple(labels.shape) != (B,) or tuple(consts.shape) != (B,):
        raise ValueError(f"labels and consts must be [{B}]")
    if check_labels and B and (int(labels.min()) < 0 or int(labels.max()) >= C):
        raise ValueError(f"labels must lie in [0, {C})")
    E = head_w.shape[1]
    dfeat = torch.empty(B, E, dtype=torch.float32, device=logits.device)
    margin = torch.empty(B, dtype=torch.float32, device=logits.device)
    other = torch.empty(B, dtype=torch.int32, device=logits.device)
    check(_lib.load().nd_margin_head_bwd(ptr(logits), ptr(labels), ptr(consts), ptr(head_w), ptr(dfeat), ptr(margin), ptr(other), B, C, E,
                                         float(confidence), _stream(logits)), "nd_margin_head_bwd")
    return dfeat, margin, other


def l2_step(x: torch.Tensor, x0: torch.Tensor, grad: Optional[torch.Tensor], alpha: float, eps: float, lo: float = 0.0, hi: float = 1.0,
            want_norms: bool = False):
    """foolbox's L2 step, project, clip per image: t = x + alpha * g / max(||g||, 1e-12), d = t - x0,
    clip(x0 + d * min(1, eps / max(||d||, 1e-12)), lo, hi).  grad None: no step -- with lo = -inf, hi = inf that is the final
    clip_perturbation.  want_norms: also (gnorm, dnorm) [B], the values the elementwise pass used (gnorm 0 without a gradient)."""
    x, x0 = _f32(x, "x"), _f32(x0, "x0")
    if x0.shape != x.shape:
        raise ValueError("x0 must have the shape of x")
    B, per = _per_image(x)
    if grad is not None:
        grad = _f32(grad, "grad")
        if grad.shape != x.shape:
            raise ValueError("grad must have the shape of x")
    out = torch.empty_like(x)
    gnorm = torch.empty(B, dtype=torch.float32, device=x.device)
    dnorm = torch.empty(B, dtype=torch.float32, device=x.device)
    check(_lib.load().nd_l2_step(ptr(x), ptr(x0), ptr(grad), ptr(out), ptr(gnorm), ptr(dnorm), ptr(_l2_ws(B, x.device)), B, per, float(alpha),
                                 float(eps), float(lo), float(hi), _stream(x)), "nd_l2_step")
    return (out, gnorm, dnorm) if want_norms else out


def l2_random_start(x0: torch.Tensor, eps: float, seed: int, first_image: int = 0, restart: int = 0, lo: float = 0.0, hi: float = 1.0,
                    want_norm: bool = False):
    """clip(x0 + eps * r, lo, hi), r uniform in the unit n-ball (foolbox's uniform_n_balls: the first n of n + 2 normals over the norm of
    all n + 2); the normals of image b are keyed on (seed, first_image + b, element, restart).  want_norm: also snorm [B]."""
    x0 = _f32(x0, "x0")
    B, per = _per_image(x0)
    out = torch.empty_like(x0)
    snorm = torch.empty(B, dtype=torch.float32, device=x0.device)
    check(_lib.load().nd_l2_random_start(ptr(x0), ptr(out), ptr(snorm), ptr(_l2_ws(B, x0.device, 1)), B, per, int(seed) & 0xFFFFFFFFFFFFFFFF,
                                         int(first_image) & 0xFFFFFFFF, int(restart) & 0xFFFFFFFF, float(eps), float(lo), float(hi),
                                         _stream(x0)), "nd_l2_random_start")
    return (out, snorm) if want_norm else out


def cw_attack_space(x0: torch.Tensor, lo: float = 0.0, hi: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(w0, xrec): w0 = atanh(((x0 - a) / b) * 0.999999), xrec = tanh(w0) * b + a, a = (lo + hi) / 2, b = (hi - lo) / 2."""
    x0 = _f32(x0, "x0")
    if x0.numel() == 0 or x0.numel() % 4:
        raise ValueError("the number of elements must be a positive multiple of 4")
    w0, xrec = torch.empty_like(x0), torch.empty_like(x0)
    check(_lib.load().nd_cw_attack_space(ptr(x0), ptr(w0), ptr(xrec), x0.numel(), float(lo), float(hi), _stream(x0)), "nd_cw_attack_space")
    return w0, xrec


class CwState:
    """Carlini & Wagner's device state for B images shaped like x0: the tanh-space variable delta with Adam's m and v, the iterate's t and x,
    best / best_norm over all binary-search steps, and the per-image scalars of an iteration (sq_rec, sq_x0, found, flags, loss)."""

    def __init__(self, x0: torch.Tensor):
        x0 = _f32(x0, "x0")
        self.B, self.per = _per_image(x0)
        dev, B = x0.device, self.B
        self.delta, self.m, self.v = torch.zeros_like(x0), torch.zeros_like(x0), torch.zeros_like(x0)
        self.t, self.x = torch.empty_like(x0), torch.empty_like(x0)
        self.best = torch.zeros_like(x0)
        self.best_norm = torch.full((B,), float("inf"), dtype=torch.float32, device=dev)
        self.sq_rec, self.sq_x0, self.loss = (torch.empty(B, dtype=torch.float32, device=dev) for _ in range(3))
        self.found, self.flags = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        self.ws = _l2_ws(B, dev)

    def reset_search_step(self) -> None:
        """The start of a binary-search step: delta = 0, Adam's state = 0, found = False (best and best_norm carry over)."""
        for t in (self.delta, self.m, self.v, self.found):
            t.zero_()


def cw_model_space(w0: torch.Tensor, x0: torch.Tensor, xrec: torch.Tensor, s: CwState, lo: float = 0.0, hi: float = 1.0) -> torch.Tensor:
    """s.t = tanh(w0 + s.delta), s.x = s.t * b + a, s.sq_rec = sum (x - xrec)^2, s.sq_x0 = sum (x - x0)^2 per image; returns s.x."""
    shape = tuple(s.delta.shape)
    w0, x0, xrec = (_inplace(t, n, shape=shape) for t, n in ((w0, "w0"), (x0, "x0"), (xrec, "xrec")))
    check(_lib.load().nd_cw_model_space(ptr(w0), ptr(s.delta), ptr(x0), ptr(xrec), ptr(s.t), ptr(s.x), ptr(s.sq_rec), ptr(s.sq_x0), ptr(s.ws),
                                        s.B, s.per, float(lo), float(hi), _stream(w0)), "nd_cw_model_space")
    return s.x


def cw_control(logits: torch.Tensor, labels: torch.Tensor, consts: torch.Tensor, margin: torch.Tensor, s: CwState,
               confidence: float = 0.0) -> torch.Tensor:
    """The per-image bookkeeping of one CW iteration (nd_cw_control), in place on s: found |= adv, best_norm, flags = new best,
    loss = consts * max(0, margin) + sq_rec.  Nothing is read back; returns s.loss."""
    logits = _f32(logits, "logits")
    if logits.dim() != 2 or logits.shape[0] != s.B:
        raise ValueError(f"logits must be [{s.B}, C]")
    B, C = logits.shape
    if C < 2 or C > 1024:
        raise ValueError(f"cw control takes 2 <= C <= 1024 classes (C={C})")
    labels = labels.to(device=logits.device, dtype=torch.int64).contiguous()
    consts, margin = _f32(consts, "consts"), _f32(margin, "margin")
    if tuple(labels.shape) != (B,) or tuple(consts.shape) != (B,) or tuple(margin.shape) != (B,):
        raise ValueError(f"labels, consts and margin must be [{B}]")
    for name in ("sq_rec", "sq_x0", "best_norm", "loss"):
        _inplace(getattr(s, name), name, torch.float32, (B,))
    for name in ("found", "flags"):
        _inplace(getattr(s, name), name, torch.int32, (B,))
    check(_lib.load().nd_cw_control(ptr(logits), ptr(labels), ptr(consts), ptr(margin), ptr(s.sq_rec), ptr(s.sq_x0), ptr(s.best_norm),
                                    ptr(s.found), ptr(s.flags), ptr(s.loss), B, C, float(confidence), _stream(logits)), "nd_cw_control")
    return s.loss


def cw_b_half(lo: float, hi: float) -> float:
    """b = (hi - lo) / 2 as nd_cw_attack_space and nd_cw_model_space form it: float32 lo and hi, float32 arithmetic (each double operation
    on float32 operands, rounded to float32, is the float32 operation).  nd_cw_update's b_half must be this value, not the double's rounding:
    at (-0.3, 1.1) the two differ by an ulp."""
    r = lambda v: ctypes.c_float(v).value                                  # noqa: E731
    return r(r(r(hi) - r(lo)) / 2.0)


def cw_update(s: CwState, dx: torch.Tensor, xrec: torch.Tensor, stepsize: float, k: int, lo: float = 0.0, hi: float = 1.0,
              use_flags: bool = True) -> None:
    """Iteration k's per-element pass (nd_cw_update), in place on s: best = x in the flagged rows, then the tanh-space gradient of
    sum_b loss_b from dx and the Adam update of delta with the bias corrections of step k + 1 (computed here in double).  dx is
    taken as it is: a non-contiguous one is refused, not copied."""
    shape = tuple(s.delta.shape)
    dx, xrec = _inplace(dx, "dx", shape=shape), _inplace(xrec, "xrec", shape=shape)
    bc1, bc2 = 1.0 - 0.9 ** (k + 1), 1.0 - 0.999 ** (k + 1)
    check(_lib.load().nd_cw_update(ptr(s.delta), ptr(s.m), ptr(s.v), ptr(dx), ptr(s.x), ptr(xrec), ptr(s.t), ptr(s.best),
                                   ptr(s.flags) if use_flags else None, s.B, s.per, float(stepsize), bc1, bc2, cw_b_half(lo, hi),
                                   _stream(dx)), "nd_cw_update")


# ---- the gradient through the mapping MLPs (include/nested_diffusion.h: nd_linear_bwd, nd_ensemble_xent_bwd; the chain: mapping.py) -----
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
    gate = _f32(gate, "gate") if gate is not None else None
    add = _f32(add, "add") if add is not None else None
    for t, name in ((gate, "gate"), (add, "add")):
        if t is not None and (tuple(t.shape) != (M, K) or t.device != dy.device):
            raise ValueError(f"{name} is {tuple(t.shape)} on {t.device}; expected [{M}, {K}] on {dy.device}")
    if weight.data.device != dy.device:
        raise ValueError(f"weight is on {weight.data.device}, dy on {dy.device}")
    out = torch.empty(M, K, dtype=torch.float32, device=dy.device)
    for s in range(0, M, LINEAR_BWD_MAX_M):
        e = min(s + LINEAR_BWD_MAX_M, M)
        check(lib.nd_linear_bwd(ptr(dy[s:e]), ptr(weight.data), ptr(gate[s:e]) if gate is not None else None,
                                ptr(add[s:e]) if add is not None else None, ptr(out[s:e]), e - s, N, K, weight.dtype, _stream(dy)),
              "nd_linear_bwd")
    return out


def ensemble_xent_grad(logits: torch.Tensor, labels: Optional[torch.Tensor] = None, check_labels: bool = True):
    """(P [B, C], loss [B], dlogits [K, B, C]) of the cross-entropy of the members' averaged softmax (nd_ensemble_xent_bwd): logits
    [K, B, C], P = mean_k softmax(logits_k), loss = -log P[b, label], dlogits_k = dloss / dlogits_k.  labels None: (P, None, None), the
    scores-only call.  check_labels=False skips the label-range check, which reads back (the kernel gives an out-of-range label a NaN loss
    and no gradient)."""
    logits = _f32(logits, "logits")
    if logits.dim() != 3:
        raise ValueError("logits must be [K, B, C]")
    K, B, C = logits.shape
    if not 1 <= K <= 32 or B < 1 or not 2 <= C <= 1024:
        raise ValueError(f"the ensemble head takes 1 <= K <= 32 members, B >= 1 and 2 <= C <= 1024 classes (K={K}, B={B}, C={C})")
    P = torch.empty(B, C, dtype=torch.float32, device=logits.device)
    loss = dlogits = None
    if labels is not None:
        labels = labels.to(device=logits.device, dtype=torch.int64).contiguous()
        if tuple(labels.shape) != (B,):
            raise ValueError(f"labels must be [{B}]")
        if check_labels and (int(labels.min()) < 0 or int(labels.max()) >= C):
            raise ValueError(f"labels must lie in [0, {C})")
        loss = torch.empty(B, dtype=torch.float32, device=logits.device)
        dlogits = torch.empty_like(logits)
    check(_lib.load().nd_ensemble_xent_bwd(ptr(logits), ptr(labels), ptr(P), ptr(loss), ptr(dlogits), K, B, C, _stream(logits)),
          "nd_ensemble_xent_bwd")
    return P, loss, dlogits


def _adam_fields(what: str, lr: float, t: int, betas: Tuple[float, float], eps: float) -> tuple:
    """The seven fields nd_adam_step and nd_adamw_step share, formed in double, as torch's Python does (ctypes rounds each to fp32 once):
    step_size = lr / (1 - beta1^t), sqrt_bc2 = sqrt(1 - beta2^t)."""
    t = int(t)
    if t < 1:
        raise ValueError(f"{what}: steps count from 1 (t={t})")
    b1, b2 = float(betas[0]), float(betas[1])
    if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0) or lr < 0.0 or eps < 0.0:
        raise ValueError(f"{what} needs lr >= 0, eps >= 0 and betas in [0, 1) (lr={lr}, betas={betas}, eps={eps})")
    return b1, 1.0 - b1, b2, 1.0 - b2, float(lr) / (1.0 - b1 ** t), (1.0 - b2 ** t) ** 0.5, float(eps)


def adam_step(lr: float, t: int, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8) -> "_lib.NdAdamStep":
    """nd_adam_step of step t >= 1 (torch.optim.Adam's `step` after its increment)."""
    return _lib.NdAdamStep(*_adam_fields("adam_step", lr, t, betas, eps))


def adamw_step(lr: float, t: int, weight_decay: float = 0.1, betas: Tuple[float, float] = (0.9, 0.999),
               eps: float = 1e-8) -> "_lib.NdAdamwStep":
    """nd_adamw_step of step t >= 1 (torch.optim.AdamW's `step` after its increment): adam_step's fields plus decay = 1 - lr *
    weight_decay, formed in double like them."""
    if weight_decay < 0.0:
        raise ValueError(f"adamw_step needs weight_decay >= 0 (weight_decay={weight_decay})")
    return _lib.NdAdamwStep(*_adam_fields("adamw_step", lr, t, betas, eps), 1.0 - float(lr) * float(weight_decay))


_STEP_ARG = {_lib.NdAdamStep: "adam", _lib.NdAdamwStep: "adamw"}


def _fused_state(step, step_type, return_grad: bool, what: str, dev, state) -> bool:
    """The checks every gradient + optimizer call shares; True when the call is fused.  step: the call's ops.adam_step / ops.adamw_step
    (a step_type), or None for the gradient-only call, which then needs return_grad.  state: (tensor-or-image, name, size) of every
    buffer the update writes in place, all distinct: a float32 contiguous tensor on `dev` of shape `size` (a tuple) or of `size` elements
    (an int), or -- `size` a PackedWeight -- a PackedWeight image of its (N, K, dtype, device)."""
    arg = _STEP_ARG[step_type]
    if step is None:
        if not return_grad:
            raise ValueError(f"{what}: {arg}=None and return_grad=False: nothing to compute")
        return False
    if not isinstance(step, step_type):
        raise TypeError(f"{arg} must be an ops.{arg}_step(...) or None")
    ptrs = set()
    for t, name, size in state:
        if isinstance(size, PackedWeight):
            if not isinstance(t, PackedWeight):
                raise TypeError(f"{name} must be a PackedWeight (weight.zeros_like())")
            if (t.N, t.K, t.dtype) != (size.N, size.K, size.dtype) or t.data.device != size.data.device:
                raise ValueError(f"{name} is a [{t.N}, {t.K}] image on {t.data.device}; expected weight's [{size.N}, {size.K}] on "
                                 f"{size.data.device}")
            t = t.data
        else:
            if t is None:
                raise ValueError(f"{what}: {name} is None in a fused call")
            shaped = isinstance(size, tuple)
            _inplace(t, name, shape=size if shaped else None)
            if (not shaped and t.numel() != size) or t.device != dev:
                raise ValueError(f"{name} has {t.numel()} elements on {t.device}; expected {size} on {dev}")
        ptrs.add(t.data_ptr())
    if len(ptrs) != len(state):
        raise ValueError(f"{what}: the parameter and moment buffers must be distinct")
    return True


def linear_wgrad_adam(dy: torch.Tensor, x: torch.Tensor, weight: PackedWeight, m: Optional[PackedWeight], v: Optional[PackedWeight], adam,
                      gscale: float = 1.0, return_grad: bool = False) -> Optional[PackedWeight]:
    """One Adam step of linear(x, weight)'s weight on the gradient gscale * (dy^T @ x), dy = dL/d(its output) [M, N], x its input [M, K]
    (nd_linear_wgrad_adam: the gradient is formed tile by tile and applied in registers, never written unless asked for).  weight, m, v
    are updated IN PLACE in their packed images: weight.data keeps its address, so whatever streams that image sees the new weights.
    adam: ops.adam_step(lr, t), or None for the gradient-only call (m, v unused).  return_grad: also return the gradient as a packed
    image (.unpack() gives [N, K]).  1 <= M <= 128."""
    lib = _lib.load()
    if not isinstance(weight, PackedWeight):
        raise TypeError("weight must be a PackedWeight (the image the forward streams)")
    if weight.dtype != _lib.ND_DTYPE_F32:
        raise _lib.NdError("linear_wgrad_adam updates fp32 weight images only: training runs in fp32 mode, not on an fp16 PackedWeight")
    dy, x = _f32(dy, "dy"), _f32(x, "x")
    if dy.dim() != 2 or dy.shape[0] < 1 or dy.shape[1] != weight.N:
        raise ValueError(f"dy is {tuple(dy.shape)}, weight is [{weight.N}, {weight.K}]: expected [M >= 1, {weight.N}]")
    M, N, K = dy.shape[0], weight.N, weight.K
    if M > LINEAR_BWD_MAX_M:
        raise ValueError(f"linear_wgrad_adam takes at most {LINEAR_BWD_MAX_M} rows per step (M={M}): a weight gradient sums over the batch, "
                         f"it cannot run as chunks")
    if K % 16:
        raise ValueError(f"K must be a multiple of 16 (K={K})")
    if tuple(x.shape) != (M, K) or x.device != dy.device:
        raise ValueError(f"x is {tuple(x.shape)} on {x.device}; expected [{M}, {K}] on {dy.device}")
    if weight.data.device != dy.device:
        raise ValueError(f"weight is on {weight.data.device}, dy on {dy.device}")
    on = _fused_state(adam, _lib.NdAdamStep, return_grad, "linear_wgrad_adam", dy.device, ((weight, "weight", weight), (m, "m", weight), (v, "v", weight)))
    g = weight.zeros_like() if return_grad else None
    check(lib.nd_linear_wgrad_adam(ptr(dy), ptr(x), ptr(weight.data), ptr(m.data) if on else None, ptr(v.data) if on else None,
                                   ptr(g.data) if g is not None else None, M, N, K, weight.dtype, float(gscale),
                                   ctypes.byref(adam) if on else None, _stream(dy)), "nd_linear_wgrad_adam")
    return g


def linear_wgrad_plan(N: int, K: int) -> dict:
    """The launch geometry of nd_linear_wgrad_adam for an [N, K] weight (host only): 16-column blocks per workgroup, workgroups over K,
    workgroups over the row blocks, row blocks per workgroup."""
    out = (ctypes.c_int * 4)()
    check(_lib.load().nd_linear_wgrad_plan(int(N), int(K), out), "nd_linear_wgrad_plan")
    return {"kb_per_wg": out[0], "grid_x": out[1], "grid_y": out[2], "rb_per_wg": out[3]}


def bias_grad_adam(dy: torch.Tensor, bias: torch.Tensor, m: Optional[torch.Tensor], v: Optional[torch.Tensor], adam, gscale: float = 1.0,
                   return_grad: bool = False) -> Optional[torch.Tensor]:
    """One Adam step of a bias [N] on the gradient gscale * dy.sum(0) (summed in the order m = 0 .. M - 1), in place (nd_bias_grad_adam).
    adam None: the gradient-only call."""
    dy = _f32(dy, "dy")
    if dy.dim() != 2 or dy.shape[0] < 1 or dy.shape[1] < 1:
        raise ValueError(f"dy is {tuple(dy.shape)}: expected [M >= 1, N >= 1]")
    M, N = dy.shape
    on = _fused_state(adam, _lib.NdAdamStep, return_grad, "bias_grad_adam", dy.device, ((bias, "bias", (N,)), (m, "m", (N,)), (v, "v", (N,))))
    g = torch.empty(N, dtype=torch.float32, device=dy.device) if return_grad else None
    check(_lib.load().nd_bias_grad_adam(ptr(dy), ptr(bias) if on else None, ptr(m) if on else None, ptr(v) if on else None, ptr(g), M, N,
                                        float(gscale), ctypes.byref(adam) if on else None, _stream(dy)), "nd_bias_grad_adam")
    return g


# ---- training of the ViT (include/nested_diffusion.h: nd_gemm_tn_adamw, nd_colsum_adamw, nd_layernorm_wgrad_adamw; the loop: train_transformer.py)
COLSUM_CHUNK = 64                                          # ND_COLSUM_CHUNK: rows per partial of the column sums


def gemm_tn_adamw(dy: torch.Tensor, x: torch.Tensor, w: Optional[torch.Tensor], m: Optional[torch.Tensor], v: Optional[torch.Tensor], adamw,
                  gscale: float = 1.0, return_grad: bool = False) -> Optional[torch.Tensor]:
    """One AdamW step of a row-major fp32 weight w [N, K] on the gradient gscale * (dy^T @ x), dy [M, N], x [M, K], any M >= 1
    (nd_gemm_tn_adamw: the gradient is formed tile by tile and applied in registers, never written unless asked for).  w, m, v are
    updated IN PLACE.  adamw: ops.adamw_step(lr, t), or None for the gradient-only call (w, m, v unused).  return_grad: also return the
    gradient [N, K]."""
    dy, x = _f32(dy, "dy"), _f32(x, "x")
    if dy.dim() != 2 or x.dim() != 2 or dy.shape[0] < 1 or dy.shape[1] < 1 or x.shape[0] != dy.shape[0] or x.device != dy.device:
        raise ValueError(f"dy is {tuple(dy.shape)} on {dy.device}, x is {tuple(x.shape)} on {x.device}: expected [M >= 1, N >= 1] and [M, K]")
    (M, N), K = dy.shape, x.shape[1]
    if K < 16 or K % 16:
        raise ValueError(f"K must be a positive multiple of 16 (K={K})")
    on = _fused_state(adamw, _lib.NdAdamwStep, return_grad, "gemm_tn_adamw", dy.device, ((w, "w", N * K), (m, "m", N * K), (v, "v", N * K)))
    g = torch.empty(N, K, dtype=torch.float32, device=dy.device) if return_grad else None
    check(_lib.load().nd_gemm_tn_adamw(ptr(dy), ptr(x), ptr(w) if on else None, ptr(m) if on else None, ptr(v) if on else None, ptr(g), M, N, K,
                                       float(gscale), ctypes.byref(adamw) if on else None, _stream(dy)), "nd_gemm_tn_adamw")
    return g


def gemm_tn_plan(N: int, K: int) -> dict:
    """The tile geometry of nd_gemm_tn_adamw for an [N, K] result (host only)."""
    out = (ctypes.c_int * 5)()
    check(_lib.load().nd_gemm_tn_plan(int(N), int(K), out), "nd_gemm_tn_plan")
    return {"tile_n": out[0], "tile_k": out[1], "m_tile": out[2], "grid_k": out[3], "grid_n": out[4]}


def colsum_adamw(dy: torch.Tensor, b: Optional[torch.Tensor], m: Optional[torch.Tensor], v: Optional[torch.Tensor], adamw,
                 gscale: float = 1.0, return_grad: bool = False) -> Optional[torch.Tensor]:
    """One AdamW step of a vector parameter b (N elements, any shape) on the gradient gscale * dy.sum(0), dy [M, N], in place
    (nd_colsum_adamw).  The sum runs over chunks of COLSUM_CHUNK rows, each in row order, the partials in chunk order.  adamw None: the
    gradient-only call, returns [N]."""
    dy = _f32(dy, "dy")
    if dy.dim() != 2 or dy.shape[0] < 1 or dy.shape[1] < 1:
        raise ValueError(f"dy is {tuple(dy.shape)}: expected [M >= 1, N >= 1]")
    M, N = dy.shape
    on = _fused_state(adamw, _lib.NdAdamwStep, return_grad, "colsum_adamw", dy.device, ((b, "b", N), (m, "m", N), (v, "v", N)))
    g = torch.empty(N, dtype=torch.float32, device=dy.device) if return_grad else None
    check(_lib.load().nd_colsum_adamw(ptr(dy), ptr(b) if on else None, ptr(m) if on else None, ptr(v) if on else None, ptr(g), M, N,
                                      float(gscale), ctypes.byref(adamw) if on else None, _stream(dy)), "nd_colsum_adamw")
    return g


def layernorm_wgrad_adamw(x: torch.Tensor, g: torch.Tensor, eps: float, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor],
                          m_gamma: Optional[torch.Tensor], v_gamma: Optional[torch.Tensor], m_beta: Optional[torch.Tensor],
                          v_beta: Optional[torch.Tensor], adamw, gscale: float = 1.0, return_grad: bool = False):
    """One AdamW step of LayerNorm's gamma and beta [dim] on gscale * (sum_r g * xhat, sum_r g), x the LayerNorm's input [rows, dim], g =
    dL/d(its output), in place (nd_layernorm_wgrad_adamw; xhat recomputed from x as nd_layernorm does).  adamw None: the gradient-only
    call, returns (dgamma, dbeta)."""
    x, g = _f32(x, "x"), _f32(g, "g")
    if x.dim() != 2 or g.shape != x.shape or g.device != x.device or x.shape[0] < 1:
        raise ValueError(f"x is {tuple(x.shape)}, g is {tuple(g.shape)}: expected two [rows >= 1, dim] tensors on one device")
    rows, dim = x.shape
    if dim < 4 or dim % 4 or dim > 2048:
        raise ValueError(f"dim must be a multiple of 4 in [4, 2048] (dim={dim})")
    names = ("gamma", "beta", "m_gamma", "v_gamma", "m_beta", "v_beta")
    on = _fused_state(adamw, _lib.NdAdamwStep, return_grad, "layernorm_wgrad_adamw", x.device,
                      [(t, n, dim) for t, n in zip((gamma, beta, m_gamma, v_gamma, m_beta, v_beta), names)])
    dg = torch.empty(dim, dtype=torch.float32, device=x.device) if return_grad else None
    db = torch.empty(dim, dtype=torch.float32, device=x.device) if return_grad else None
    p = [ptr(t) if on else None for t in (gamma, beta, m_gamma, v_gamma, m_beta, v_beta)]
    lib = _lib.load()
    ws = _workspace(lib.nd_layernorm_wgrad_workspace_bytes(rows, dim), x.device)      # the per-chunk partials
    check(lib.nd_layernorm_wgrad_adamw(ptr(x), ptr(g), *p, ptr(dg), ptr(db), rows, dim, float(eps), float(gscale),
                                       ctypes.byref(adamw) if on else None, ptr(ws), ws.numel(), _stream(x)), "nd_layernorm_wgrad_adamw")
    return (dg, db) if return_grad else None


# ---- training of the noise estimators (include/nested_diffusion.h: nd_bn_train_fwd / _bwd, nd_qsample, nd_mse_grad, nd_sumsq, nd_clip_adam;
# the loop: train_diffusion.py) ----
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
    for p, name in ((gamma, "gamma"), (beta, "beta")):
        if tuple(p.shape) != (N,) or p.device != u.device:
            raise ValueError(f"{name} is {tuple(p.shape)} on {p.device}; expected [{N}] on {u.device}")
    if (table is None) != (t is None):
        raise ValueError(f"{what}: table and t come together")
    rows_table = 0
    if table is not None:
        table = _f32(table, "table")
        if table.dim() != 2 or table.shape[0] < 1 or table.shape[1] != N or table.device != u.device:
            raise ValueError(f"table is {tuple(table.shape)} on {table.device}; expected [rows >= 1, {N}] on {u.device}")
        if not t.is_cuda or t.dtype != torch.int32 or tuple(t.shape) != (M,) or t.device != u.device:
            raise ValueError(f"t must be an int32 GPU tensor [{M}] on {u.device} (checked against the table on the host before the upload)")
        t, rows_table = t.contiguous(), table.shape[0]
    if mul is not None:
        mul = _f32(mul, "mul")
        if tuple(mul.shape) != (M, N) or mul.device != u.device:
            raise ValueError(f"mul is {tuple(mul.shape)} on {mul.device}; expected [{M}, {N}] on {u.device}")
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
    for p, name, shape in ((xhat, "xhat", (M, N)), (rstd, "rstd", (N,))):
        if tuple(p.shape) != shape or p.device != dout.device:
            raise ValueError(f"{name} is {tuple(p.shape)} on {p.device}; expected {list(shape)} on {dout.device}")
    if table is not None:
        if u is None:
            raise ValueError("bn_train_backward: the gain needs u, the Linear's output")
        u = _f32(u, "u")
        if tuple(u.shape) != (M, N) or u.device != dout.device:
            raise ValueError(f"u is {tuple(u.shape)} on {u.device}; expected [{M}, {N}] on {dout.device}")
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
        if tuple(p.shape) != (M, C) or p.device != first.device:
            raise ValueError(f"{name} is {tuple(p.shape)} on {p.device}; expected [{M}, {C}] on {first.device}")
    return M, C


def qsample(y0: torch.Tensor, yhat: torch.Tensor, e: torch.Tensor, ca: torch.Tensor, cb: torch.Tensor) -> torch.Tensor:
    """q_sample with per-row coefficients gathered on the HOST (nd_qsample): ca[r] * y0 + (1 - ca[r]) * yhat + cb[r] * e; y0, yhat, e
    [M, C], ca = alphas_bar_sqrt[t], cb = one_minus_alphas_bar_sqrt[t] as float32 [M]."""
    y0, yhat, e, ca, cb = _f32(y0, "y0"), _f32(yhat, "yhat"), _f32(e, "e"), _f32(ca, "ca"), _f32(cb, "cb")
    M, C = _rows_by_classes("qsample", ((y0, "y0"), (yhat, "yhat"), (e, "e")))
    for p, name in ((ca, "ca"), (cb, "cb")):
        if tuple(p.shape) != (M,) or p.device != y0.device:
            raise ValueError(f"{name} is {tuple(p.shape)} on {p.device}; expected [{M}] on {y0.device}")
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


def clip_adam(w, m, v, g, adam, sumsq: Optional[torch.Tensor] = None, max_norm: float = 1.0) -> None:
    """clip_grad_norm_'s scaling by min(1, max_norm / (sqrt(sumsq) + 1e-6)) and one Adam step on a materialised gradient, in place on w,
    m, v (nd_clip_adam).  w, m, v, g: four float32 GPU tensors of one shape, or four PackedWeight images of one shape (elementwise: the
    layout does not matter).  sumsq: the device scalar ops.sumsq accumulated over ALL gradients, or None for no clipping."""
    if not isinstance(adam, _lib.NdAdamStep):
        raise TypeError("adam must be an ops.adam_step(...)")
    if isinstance(w, PackedWeight):
        for p, name in ((m, "m"), (v, "v"), (g, "g")):
            if not isinstance(p, PackedWeight) or (p.N, p.K, p.dtype) != (w.N, w.K, w.dtype):
                raise ValueError(f"{name} must be a PackedWeight image of w's shape [{w.N}, {w.K}]")
        if w.dtype != _lib.ND_DTYPE_F32:
            raise _lib.NdError("clip_adam updates fp32 weight images only")
        w, m, v, g = w.data, m.data, v.data, g.data
    g = _f32(g, "g")
    for p, name in ((w, "w"), (m, "m"), (v, "v")):
        _inplace(p, name, shape=tuple(g.shape))
        if p.device != g.device:
            raise ValueError(f"{name} is on {p.device}, g on {g.device}")
    if len({w.data_ptr(), m.data_ptr(), v.data_ptr(), g.data_ptr()}) != 4:
        raise ValueError("clip_adam: w, m, v and g must be distinct buffers")
    if g.numel() < 1:
        raise ValueError("clip_adam of an empty tensor")
    if sumsq is not None:
        sumsq = _f32(sumsq, "sumsq")
        if sumsq.numel() != 1 or sumsq.device != g.device:
            raise ValueError(f"sumsq must be one float32 on {g.device}")
    check(_lib.load().nd_clip_adam(ptr(w), ptr(m), ptr(v), ptr(g), g.numel(), ptr(sumsq), float(max_norm), ctypes.byref(adam), _stream(g)),
          "nd_clip_adam")
