"""The conditioner: ViT prefix blocks + mapping MLPs -> latent conditions (guiding predictions), its gradient, and the attack target on it.

Mirrors Diffusion.compute_guiding_prediction (classification_train_separately.py:330-348).  Difference from the reference that does not
change results: member i's prefix blocks[0..i-1] reuse member i-1's tokens instead of recomputing from patch_embed (15 -> 5 block
evaluations; eval-mode blocks are deterministic functions of their input)."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import torch

from .. import _lib, ops
from .._lib import check, ptr
from .mlp import Classifier
from .vit import LN_EPS, VisionTransformer, check_backward_tokens, require_fp32_split


class GuidingConditioner:
    """cond_pred_model {'vit', 'mlps'} of the reference runner (classification_train_separately.py:249-275).

    compute_guiding_prediction is ONE call into the library (nd_guiding_prediction): patch_embed, the shared prefix blocks and
    every mapping MLP are sequenced in C on the current stream.  The handle (`nd_cond`) holds pointers into the tensors of
    `vit` and `mlps` (kept alive here) and one workspace for the activations."""

    def __init__(self, vit: VisionTransformer, mlps: Sequence[Classifier]):
        self.vit, self.mlps = vit, list(mlps)
        if not self.mlps:
            raise ValueError("at least one mapping MLP is required")
        if len(self.mlps) > vit.depth:
            raise ValueError(f"{len(self.mlps)} mapping MLPs need as many ViT blocks, the ViT has {vit.depth}")
        self._h = None
        self._key = None
        self._ws = None

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _lib.load().nd_cond_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def handle(self, B: int, img_size: int):
        """nd_cond for batches of up to B images of img_size x img_size (created on first use, re-created when either grows)."""
        if self._h is not None and self._key[0] >= B and self._key[1] == img_size:
            return self._h
        lib = _lib.load()
        vit, m0 = self.vit, self.mlps[0]
        if img_size % vit.patch:
            raise ValueError(f"image size {img_size} is not a multiple of the patch size {vit.patch}")
        n_tok = (img_size // vit.patch) ** 2
        widths = [m0.p[f"linear{i}.weight"].N for i in (1, 2, 3)]
        n_cls = m0.p["linear4.weight"].N
        dt = _lib.dtype_code(vit.dtype)
        for m in self.mlps:
            if [m.p[f"linear{i}.weight"].N for i in (1, 2, 3)] != widths or m.p["linear4.weight"].N != n_cls \
                    or m.in_features != n_tok * vit.embed_dim or m.p["linear1.weight"].dtype != dt:
                raise ValueError("mapping MLPs must share one shape / dtype and read all tokens of a ViT block")
        cfg = _lib.NdCondConfig()
        cfg.img_size, cfg.patch, cfg.in_chans, cfg.embed_dim, cfg.num_heads = img_size, vit.patch, vit.in_chans, vit.embed_dim, vit.num_heads
        cfg.mlp_hidden = vit.p["blocks.0.mlp.fc1.weight"].shape[0]
        cfg.n_blocks, cfg.n_mlps = vit.depth, len(self.mlps)
        cfg.mlp_widths[0], cfg.mlp_widths[1], cfg.mlp_widths[2] = widths
        cfg.num_classes, cfg.max_batch, cfg.max_tokens, cfg.ln_eps = n_cls, max(B, 1), n_tok + 1, LN_EPS
        cfg.operand_dtype = _lib.ND_DTYPE_F32_SPLIT if vit.split else dt

        def dptr(v):
            return v.data.data_ptr() if isinstance(v, ops.SplitMatrix) else v.data_ptr()
        h = C.c_void_p()
        check(lib.nd_cond_create(C.byref(cfg), C.byref(h)), "nd_cond_create")
        nbytes = lib.nd_cond_workspace_bytes(C.byref(cfg))
        ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=vit.device)
        check(lib.nd_cond_bind_workspace(h, (ws.data_ptr() + 255) & ~255, nbytes), "nd_cond_bind_workspace")
        pe = _lib.NdPatchEmbedWeights(dptr(vit.pe_w), vit.p["patch_embed.proj.bias"].data_ptr())
        check(lib.nd_cond_set_patch_embed(h, C.byref(pe)), "nd_cond_set_patch_embed")
        for i in range(vit.depth):
            w = _lib.NdVitBlockWeights()
            for field, key in _lib.VIT_BLOCK_FIELDS:
                setattr(w, field, dptr(vit.p[f"blocks.{i}.{key}"]))
            check(lib.nd_cond_set_block(h, i, C.byref(w)), "nd_cond_set_block")
        for i, m in enumerate(self.mlps):
            w = _lib.NdMlpWeights()
            for l in range(4):
                w.w_packed[l] = m.p[f"linear{l + 1}.weight"].data.data_ptr()
                w.bias[l] = m.p[f"linear{l + 1}.bias"].data_ptr()
            check(lib.nd_cond_set_mlp(h, i, C.byref(w)), "nd_cond_set_mlp")
        if self._h is not None:
            lib.nd_cond_destroy(self._h)
        self._h, self._key, self._ws = h, (max(B, 1), img_size), ws
        return h

    def compute_guiding_prediction(self, x: torch.Tensor, include_full_vit: bool = True) -> List[torch.Tensor]:
        """classification_train_separately.py:330-348: list of K (+1) logits [B, C]."""
        x = ops._f32(x, "x")
        B, K = x.shape[0], len(self.mlps)
        h = self.handle(B, x.shape[-1])
        n_cls = self.mlps[0].p["linear4.weight"].N
        logits = torch.empty(K, B, n_cls, dtype=torch.float32, device=x.device)
        check(_lib.load().nd_guiding_prediction(h, ptr(x), ptr(logits), None, B, _lib.current_stream_ptr(x.device)),
              "nd_guiding_prediction")
        out = list(logits.unbind(0))
        if include_full_vit:
            out.append(self.vit.forward(x))          # the never-sampled (K+1)-th element (:346, quirk Q1)
        return out

    def compute_guiding_prediction_py(self, x: torch.Tensor, include_full_vit: bool = True, side_stream=None,
                                      side_work=None) -> List[torch.Tensor]:
        """The same sequence launched operator by operator from Python (tests: must equal the C-level call bit for bit; tools:
        the two-stream experiment of DESIGN 7b-6 -- with `side_stream` the HBM-bound mapping MLPs and `side_work` run beside
        the MFMA-bound ViT blocks; measured slower, not used by the product path)."""
        B = x.shape[0]
        out: List[torch.Tensor] = [None] * len(self.mlps)
        main = torch.cuda.current_stream(x.device)
        if side_stream is not None:
            side_stream.wait_stream(main)
            if side_work is not None:
                with torch.cuda.stream(side_stream):
                    side_work()
        elif side_work is not None:
            side_work()
        tok = self.vit.patch_embed(x)
        for i in range(1, len(self.mlps) + 1):
            tok = self.vit.block(i - 1, tok, B)       # prefix shared across members
            if side_stream is not None:
                ev = torch.cuda.Event()
                ev.record(main)
                tok.record_stream(side_stream)
                with torch.cuda.stream(side_stream):
                    side_stream.wait_event(ev)
                    out[i - 1] = self.mlps[i - 1](tok)
            else:
                out[i - 1] = self.mlps[i - 1](tok)
        if include_full_vit:
            out.append(self.vit.forward(x))
        if side_stream is not None:
            main.wait_stream(side_stream)
        return out

    # ---- input gradient of the mapping networks themselves (the white-box attacks on the defence's front end) ---------------------------
    def _members(self, members) -> List[int]:
        members = list(range(len(self.mlps))) if members is None else [int(m) for m in members]
        if not members or len(set(members)) != len(members) or min(members) < 0 or max(members) >= len(self.mlps):
            raise ValueError(f"members must be distinct indices in [0, {len(self.mlps)}), at least one (got {members})")
        return members

    def input_grad(self, x: torch.Tensor, labels: torch.Tensor, members: Optional[Sequence[int]] = None, check_labels: bool = True):
        """(P, dx, loss, logits) of the members the ensemble is conditioned on (member k: patch_embed -> blocks[0..k] -> mlps[k] -> softmax):
        P [B, C] = the selected members' averaged softmax, loss [B] = -log P[b, label], dx = d(loss.sum()) / dx [B, 3, H, W], logits
        [len(members), B, C] in the order of `members` (default: all).  The forward is compute_guiding_prediction_py's launches in its order
        (the logits equal compute_guiding_prediction's bit for bit); the backward is ONE chain down the shared prefix from the deepest
        selected member: each member's dlogits go through its MLP (Classifier.input_grad) and join the running token gradient at its
        level before that level's block gradient.  fp32 (split) form only.  After the optional label check nothing is read back."""
        logits, tape = self.forward_recorded(x, members)
        P, loss, dlogits = ops.ensemble_xent_grad(logits, labels, check_labels=check_labels)
        return P, self.backward(tape, dlogits), loss, logits

    def forward_recorded(self, x: torch.Tensor, members: Optional[Sequence[int]] = None) -> Tuple[torch.Tensor, dict]:
        """The first half of input_grad, for callers that put their own loss at the heads (ensemble_grad.EnsembleTarget): (logits
        [len(members), B, C] in the order of `members`, tape).  The tape holds what backward needs and is used up by it.  Every refusal of
        input_grad is made here, before anything is launched."""
        vit = self.vit
        members = self._members(members)
        x = ops._f32(x, "x")
        if x.dim() != 4:
            raise ValueError("x must be [B, C, H, W]")
        B, _, H, W = x.shape
        n_tok = (H // vit.patch) * (W // vit.patch)
        check_backward_tokens(n_tok)
        require_fp32_split("input_grad", vit=vit, mlps=self.mlps)
        vit.transposed_weights()
        top = max(members)
        tok, recs, heads = vit.patch_embed(x), [], {}
        for i in range(top + 1):
            recs.append({})
            tok = vit.block(i, tok, B, rec=recs[-1])
            if i in members:
                heads[i] = self.mlps[i].forward_recorded(tok)
        logits = torch.stack([heads[m][0] for m in members])
        return logits, dict(members=members, recs=recs, heads=heads, shape=(B, H, W, n_tok))

    def backward(self, tape: dict, dlogits: torch.Tensor, add: Optional[torch.Tensor] = None) -> torch.Tensor:
        """dx [B, 3, H, W] from dlogits [len(members), B, C] = dL/d(forward_recorded's logits): ONE chain down the shared prefix (input_grad's
        docstring).  add [B, 3 * H * W]: a gradient that reaches the image by another path (the noise estimators' encoder_x); it joins dx
        through the image-add kernel (nd_img_add_noise with std = 1: dx + add, one rounding).  The tape's activations are released level by
        level."""
        vit = self.vit
        members, recs, heads = tape["members"], tape["recs"], tape["heads"]
        B, H, W, n_tok = tape["shape"]
        dlogits = ops._f32(dlogits, "dlogits")
        n_cls = self.mlps[0].p["linear4.weight"].N
        if tuple(dlogits.shape) != (len(members), B, n_cls):
            raise ValueError(f"dlogits is {tuple(dlogits.shape)}; expected {[len(members), B, n_cls]}")
        if add is not None:
            add = ops._f32(add, "add")
            if tuple(add.shape) != (B, vit.in_chans * H * W) or add.device != dlogits.device:
                raise ValueError(f"add is {tuple(add.shape)} on {add.device}; expected {[B, vit.in_chans * H * W]} on {dlogits.device}")
        top = max(members)
        dtok, dimg = None, None
        for i in range(top, -1, -1):
            if i in heads:
                join = dtok.reshape(B, -1) if dtok is not None else None
                dtok = self.mlps[i].input_grad(dlogits[members.index(i)], heads.pop(i)[1], add=join).reshape(B * n_tok, vit.embed_dim)
                dimg = ops.split_rows(dtok)
            dtok, dimg = vit._block_grad(i, recs[i], dtok, dimg, B)
            recs[i] = None
        dx = vit._patch_embed_backward(dimg, B, H, W)
        if add is None:
            return dx
        from ..perturb import add_noise
        return add_noise(dx, 1.0, z=add.reshape(dx.shape))


class ConditionerTarget:
    """What the gradient attacks take as their model when the mapping networks themselves are attacked: .device, forward(x) -> the
    selected members' averaged softmax P [B, C] (scores; the attacks use only their argmax) and input_grad(x, labels) -> (P, dx, loss).
    It deliberately has no attribute called `vit`: attack._vit would unwrap it and attack the full ViT's head instead."""

    def __init__(self, cond: GuidingConditioner, members: Optional[Sequence[int]] = None):
        self.cond = cond
        self.members = None if members is None else cond._members(members)
        self.device = cond.vit.device

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """P [B, C]: the C-level compute_guiding_prediction, then the scores-only head call on the selected members.  That one library call
        runs EVERY member, so a subset still streams all the mapping MLPs' weights in a forward (input_grad stops at max(members))."""
        out = self.cond.compute_guiding_prediction(x, include_full_vit=False)
        sel = out if self.members is None else [out[m] for m in self.members]
        return ops.ensemble_xent_grad(torch.stack(sel))[0]

    __call__ = forward

    def input_grad(self, x: torch.Tensor, labels: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        P, dx, loss, _ = self.cond.input_grad(x, labels, self.members)
        return P, dx, loss

    def input_grad_margin(self, *args, **kwargs):
        raise NotImplementedError("Carlini-Wagner (CarliniWagner) is not implemented on a ConditionerTarget: its margin loss is defined on the "
                                  "full ViT's logits, not on the members' averaged probabilities")
