"""The ViT: the timm 0.4.12 vit_base_patch16_224 pieces the path calls (patch_embed, pos_drop, blocks[j], full forward) with the whole
backward chain the attacks and the trainer share, and the two refusals every gradient path makes before it launches anything."""
from __future__ import annotations

import os
from typing import Dict, Optional, Tuple

import torch

from .. import _lib, ops

LN_EPS = 1e-6  # timm 0.4.12: norm_layer = partial(nn.LayerNorm, eps=1e-6)


def _mfma_f32() -> bool:
    return os.environ.get("ND_GEMM_F32", "b9") == "mfma_f32"


def require_fp32_split(who: str, dtype=None, vit=None, mlps=()) -> None:
    """The refusal of everything that reads the frag32b3 weight images (the gradient chains, the trainers, the ensemble target), from
    whichever of these the caller has at that point: an operand dtype, a ViT, the mapping MLPs.  Refused: fp16 operands anywhere; a ViT
    that holds no images (it keeps the form it was built in, so it alone is asked, and no gradient call reads the environment); and,
    where no ViT is built yet, ND_GEMM_F32=mfma_f32."""
    if (dtype is not None and _lib.dtype_code(dtype) != _lib.ND_DTYPE_F32) or getattr(vit, "dtype", "f32") != "f32":
        why = "not in fp16 mode (fp16 operands)"
    elif any(getattr(m, "p", None) is not None and m.p["linear1.weight"].dtype != _lib.ND_DTYPE_F32 for m in mlps):
        why = "not in fp16 mode (the mapping MLPs hold fp16 images)"
    elif vit is not None:
        if vit.split:
            return
        why = "the ViT holds no frag32b3 images (built with ND_GEMM_F32=mfma_f32, or a GEMM depth is no multiple of 32)"
    elif _mfma_f32():
        why = "not with ND_GEMM_F32=mfma_f32"
    else:
        return
    raise _lib.NdError(f"{who} runs in the default fp32 (split) form only: {why}")


def check_backward_tokens(n_tok: int, image: tuple = ()) -> None:
    """The attention backward's token limit, refused before the forward runs, not by the first attention backward after it.  The callers
    count differently on purpose: the full ViT's path includes the cls token, the conditioner's prefix has none."""
    if n_tok > ops.ATTENTION_BWD_MAX_TOKENS:
        of = " for {} x {} images, patch {}".format(*image) if image else ""
        raise _lib.NdError(f"input_grad: the attention backward takes N <= {ops.ATTENTION_BWD_MAX_TOKENS} tokens per image (N={n_tok}{of})")


class VisionTransformer:
    """The subset of timm 0.4.12 VisionTransformer the path touches, over a timm state_dict."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], num_heads: int = 12, device="cuda", dtype="f32"):
        """dtype 'f16' (fp16 mode, not a reference mode): the Linear / patch-embedding weights are held in fp16 and the GEMMs and
        the attention contractions run on fp16 operands (fp32 accumulation, LayerNorm, softmax, residual stream)."""
        self.device = torch.device(device)
        self.dtype = "f16" if _lib.dtype_code(dtype) == _lib.ND_DTYPE_F16 else "f32"
        self.p = {k: v.detach().to(self.device, torch.float32).contiguous() for k, v in state_dict.items()
                  if torch.is_tensor(v) and v.is_floating_point()}
        w = self.p["patch_embed.proj.weight"]
        self.embed_dim, self.in_chans, self.patch = w.shape[0], w.shape[1], w.shape[-1]
        self.pe_w = w.reshape(self.embed_dim, -1).contiguous()
        gemm_keys = [k for k in self.p if k.startswith("blocks.") and
                     k.endswith(("attn.qkv.weight", "attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight"))]
        # fp32 mode: the Linear layers run on the bf16 matrix pipe with exact fp32 products (nd_gemm_split) wherever the shapes allow
        # it (every GEMM depth a multiple of 32: 768 / 3072 / 3*16*16 for ViT-B/16); the weights are then held as frag32b3 images
        # ONLY.  ND_GEMM_F32=mfma_f32 keeps the f32-input-MFMA kernels (and row-major fp32 weights).
        self.split = (self.dtype == "f32" and not _mfma_f32() and self.pe_w.shape[1] % 32 == 0
                      and all(self.p[k].shape[1] % 32 == 0 for k in gemm_keys))
        if self.split:
            self.pe_w = ops.split_rows(self.pe_w)
            for k in gemm_keys:
                self.p[k] = ops.split_rows(self.p[k])
        if self.dtype == "f16":
            self.pe_w = self.pe_w.half()
            for k in gemm_keys:
                self.p[k] = self.p[k].half()
        self.num_heads = num_heads
        self.depth = 1 + max(int(k.split(".")[1]) for k in self.p if k.startswith("blocks."))
        if self.embed_dim // num_heads != 64:
            raise ValueError("head dim must be 64 (vit_base_patch16_224: 768 / 12)")

    def patch_embed(self, x: torch.Tensor) -> torch.Tensor:
        """PatchEmbed.forward -> tokens [B*N, embed]; pos_drop is the identity in eval."""
        cols = ops.patchify(x, self.patch)
        return ops.gemm_bias_act(cols, self.pe_w, self.p["patch_embed.proj.bias"])

    def block(self, i: int, tok: torch.Tensor, B: int, rec: Optional[dict] = None) -> torch.Tensor:
        """Block.forward on tokens [B*N, embed].  rec (input_grad): a dict that receives what the backward needs -- the block input x,
        the fp32 qkv, the attention output o, the mid-block tokens x2 and the fc1 pre-activation u.  fc1 then runs without its
        activation and the GELU follows as its own kernel (the epilogue's expression, written as the fc2 operand image): same values."""
        p, pre = self.p, f"blocks.{i}."
        N = tok.shape[0] // B
        x = tok
        h = ops.layernorm(tok, p[pre + "norm1.weight"], p[pre + "norm1.bias"], LN_EPS)
        if self.split and ops.qkv_images_supported(N, self.num_heads) and not os.environ.get("ND_ATT_F32"):
            # attention on the bf16 matrix pipe as well: the qkv Linear writes the attention kernel's operand images (nd_vit_block's sequence)
            img = ops.gemm_split_qkv(ops.split_rows(h), p[pre + "attn.qkv.weight"], p[pre + "attn.qkv.bias"], B, N, self.num_heads)
            a = ops.attention_images(img, B, N, self.num_heads)
            qkv = ops.gemm_bias_act(h, p[pre + "attn.qkv.weight"], p[pre + "attn.qkv.bias"]) if rec is not None else None
        else:
            qkv = ops.gemm_bias_act(h, p[pre + "attn.qkv.weight"], p[pre + "attn.qkv.bias"])
            a = ops.attention(qkv, B, N, self.num_heads, self.dtype)
        tok = ops.gemm_bias_act(a, p[pre + "attn.proj.weight"], p[pre + "attn.proj.bias"], residual=tok)
        h = ops.layernorm(tok, p[pre + "norm2.weight"], p[pre + "norm2.bias"], LN_EPS)
        if rec is None:
            h = ops.gemm_bias_act(h, p[pre + "mlp.fc1.weight"], p[pre + "mlp.fc1.bias"], act="gelu")
            return ops.gemm_bias_act(h, p[pre + "mlp.fc2.weight"], p[pre + "mlp.fc2.bias"], residual=tok)
        u = ops.gemm_bias_act(h, p[pre + "mlp.fc1.weight"], p[pre + "mlp.fc1.bias"])
        rec.update(x=x, qkv=qkv, o=a, x2=tok, u=u)
        return ops.gemm_split(ops.gelu_split(u), p[pre + "mlp.fc2.weight"], p[pre + "mlp.fc2.bias"], residual=tok)

    def _tokens(self, x: torch.Tensor) -> torch.Tensor:
        """patch_embed + cls token + pos_embed -> [B*N, embed]"""
        B = x.shape[0]
        tok = self.patch_embed(x).reshape(B, -1, self.embed_dim)
        tok = torch.cat((self.p["cls_token"].expand(B, -1, -1), tok), dim=1) + self.p["pos_embed"]
        return tok.reshape(-1, self.embed_dim).contiguous()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """Full VisionTransformer.forward (cls token + pos_embed, all blocks, norm, head on cls).
        Only feeds the never-sampled last element of compute_guiding_prediction."""
        B = x.shape[0]
        tok = self._tokens(x)
        N = tok.shape[0] // B
        for i in range(self.depth):
            tok = self.block(i, tok, B)
        return self._head(tok, B, N)[0]

    __call__ = forward

    def _head(self, tok: torch.Tensor, B: int, N: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """The tail of the forward: the cls token's row, the final norm, the head -> (logits, cls_in = the row the norm read)."""
        cls_in = tok.reshape(B, N, self.embed_dim)[:, 0].contiguous()
        cls = ops.layernorm(cls_in, self.p["norm.weight"], self.p["norm.bias"], LN_EPS)
        return ops.linear(cls, self.p["head.weight"], self.p["head.bias"]), cls_in

    # ---- input gradient (the Linf attacks of attack.py) ------------------------------------------------------------------------
    def transposed_weights(self) -> Dict[str, "ops.SplitMatrix"]:
        """frag32b3 images of W^T for every Linear layer and the patch embedding: the weight operands of the input-gradient GEMMs
        (dX = dY . W).  Built once, on the first gradient request (~0.5 GB for ViT-B/16); a ViT that is never attacked never holds them."""
        if getattr(self, "_wT", None) is None:
            require_fp32_split("input_grad", vit=self)
            wT = {}
            for k, w in list(self.p.items()) + [("patch_embed", self.pe_w)]:
                if isinstance(w, ops.SplitMatrix):
                    wT[k] = ops.split_rows(ops.join_rows(w).t().contiguous())
            self._wT = wT
        return self._wT

    def _block_grad(self, i: int, r: dict, dy: torch.Tensor, dy_img: "ops.SplitMatrix", B: int, keep: Optional[dict] = None):
        """dL/d(block input) from dy = dL/d(block output): fp32 and its frag32b3 image.  keep (training): a dict that receives the fp32
        gradients the weight gradients read -- du (fc1's output), dh2 (norm2's), dx2 (attn.proj's), dqkv (attn.qkv's), dh1 (norm1's); the
        GELU and attention gradients then write fp32 beside their images.  None (the attacks): images only there, the same launches."""
        wT, p, pre = self._wT, self.p, f"blocks.{i}."
        N = dy.shape[0] // B
        kept = keep is not None
        dg = ops.gemm_split(dy_img, wT[pre + "mlp.fc2.weight"])
        du = ops.gelu_grad_split(r["u"], dg, want_out=kept)                     # the image, or (fp32, image)
        dh2 = ops.gemm_split(du[1] if kept else du, wT[pre + "mlp.fc1.weight"])
        dx2, dx2_img = ops.layernorm_grad(r["x2"], p[pre + "norm2.weight"], dh2, LN_EPS, residual=dy, want_split=True)
        da = ops.gemm_split(dx2_img, wT[pre + "attn.proj.weight"])
        dqkv = ops.attention_grad(r["qkv"], r["o"], da, B, N, self.num_heads, want_out=kept, want_split=True)
        dh1 = ops.gemm_split(dqkv[1] if kept else dqkv, wT[pre + "attn.qkv.weight"])
        if kept:
            keep.update(du=du[0], dh2=dh2, dx2=dx2, dqkv=dqkv[0], dh1=dh1)
        return ops.layernorm_grad(r["x"], p[pre + "norm1.weight"], dh1, LN_EPS, residual=dx2, want_split=True)

    def _forward_recorded(self, x: torch.Tensor):
        """The forward of forward(), same kernels in the same order, keeping what the input gradient needs:
        (logits, cls_in, recs, B, N, H, W)."""
        x = ops._f32(x, "x")
        B, _, H, W = x.shape
        check_backward_tokens((H // self.patch) * (W // self.patch) + 1, (H, W, self.patch))
        self.transposed_weights()
        tok = self._tokens(x)
        N = tok.shape[0] // B
        recs = []
        for i in range(self.depth):
            recs.append({})
            tok = self.block(i, tok, B, rec=recs[-1])
        logits, cls_in = self._head(tok, B, N)
        return logits, cls_in, recs, B, N, H, W

    def _token_backward(self, dcls: torch.Tensor, cls_in: torch.Tensor, recs: list, B: int, N: int, per_block=None) -> torch.Tensor:
        """dL/d(the tokens entering block 0) [B*N, embed] from dcls = dL/d(the final norm's output on the cls token): the backward chain
        every head gradient and the trainer share.  recs[i] is released once block i is behind.  per_block (training): called as
        per_block(i, rec, dy, kept) right after the chain launches of each stage, top down, with dy = dL/d(that stage's output) -- first
        for the final norm (i = depth, rec and kept None, dy = dcls), then for every block (rec = recs[i], kept = _block_grad's keep); the
        trainer issues its weight-gradient launches from it.  None: no fp32 gradient is kept."""
        dcls_in = ops.layernorm_grad(cls_in, self.p["norm.weight"], dcls, LN_EPS)
        if per_block is not None:
            per_block(self.depth, None, dcls, None)
        dy = torch.zeros(B, N, self.embed_dim, dtype=torch.float32, device=dcls.device)
        dy[:, 0] = dcls_in                                    # only the cls token reaches the head
        dy = dy.reshape(B * N, self.embed_dim)
        dy_img = ops.split_rows(dy)
        for i in reversed(range(self.depth)):
            kept = {} if per_block is not None else None
            dx, dx_img = self._block_grad(i, recs[i], dy, dy_img, B, kept)
            if per_block is not None:
                per_block(i, recs[i], dy, kept)
            dy, dy_img = dx, dx_img
            recs[i] = None
        return dy

    def _input_backward(self, dcls: torch.Tensor, cls_in: torch.Tensor, recs: list, B: int, N: int, H: int, W: int) -> torch.Tensor:
        """dL/dx from dcls: _token_backward, then the patch embedding's input gradient."""
        dy = self._token_backward(dcls, cls_in, recs, B, N)
        dpatch = dy.reshape(B, N, self.embed_dim)[:, 1:].reshape(-1, self.embed_dim).contiguous()   # cls token / pos_embed: no input path
        return self._patch_embed_backward(dpatch, B, H, W)

    def _patch_embed_backward(self, dpatch, B: int, H: int, W: int) -> torch.Tensor:
        """dL/dx [B, 3, H, W] from dL/d(patch_embed's output rows) [B * (N - 1), embed], fp32 or its frag32b3 image."""
        dcols = ops.gemm_split(dpatch, self._wT["patch_embed"])
        return ops.unpatchify(dcols, B, self.in_chans, H, W, self.patch)

    def input_grad(self, x: torch.Tensor, labels: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(logits, dx, loss): the forward (the same kernels in the same order as forward(): its logits equal forward(x) bit for bit),
        then the gradient of crossentropy(logits, labels).sum() -- foolbox's loss -- with respect to the input image x [B, 3, H, W],
        and the per-image cross-entropy."""
        logits, cls_in, recs, B, N, H, W = self._forward_recorded(x)
        dcls, loss = ops.xent_head_grad(logits, labels, self.p["head.weight"])
        return logits, self._input_backward(dcls, cls_in, recs, B, N, H, W), loss

    def input_grad_margin(self, x: torch.Tensor, labels: torch.Tensor, consts: torch.Tensor, confidence: float = 0.0,
                          check_labels: bool = True) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(logits, dx, margin): input_grad's forward and backward chain with Carlini & Wagner's loss at the head: dx is the gradient of
        sum_b consts[b] * max(0, margin[b]) with respect to x, margin = logits[label] - max over the other logits + confidence
        (nd_margin_head_bwd; a row whose margin is <= 0 has dx = 0).  check_labels=False skips the label-range check, the call's only
        read-back."""
        logits, cls_in, recs, B, N, H, W = self._forward_recorded(x)
        dcls, margin, _ = ops.margin_head_grad(logits, labels, consts, self.p["head.weight"], confidence, check_labels=check_labels)
        return logits, self._input_backward(dcls, cls_in, recs, B, N, H, W), margin
