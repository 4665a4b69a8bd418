"""Edge shapes and production batches of the input-gradient and Linf-attack kernels (csrc/nd_vit_grad.hip, csrc/nd_attack_linf.hip) and of
VisionTransformer.input_grad: the places where the kernels change behaviour (ragged query slices, the dK / dV accumulator that alone
covers keys 192..207, every LayerNorm-backward instantiation, wide and confident heads, the grid-stride loops of the element-wise kernels)
and the make_attacks batch of 32 ViT-B/16 images.

References: torch autograd in float64 on the same fp32 inputs, at the bars of tests/test_gpu_attack.py.  In the ill-conditioned regimes
(peaked attention, constant or far-off-centre LayerNorm rows, confident logits) no fixed bar fits: there the kernel must also stay within
4x of torch's own fp32 autograd, both measured against float64 (`within_fp32`).  Exact paths are checked bit for bit.  Kernel outputs are
written through the C ABI into buffers filled with 0xFF bytes first, so that an element a kernel leaves unwritten reads as NaN."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_cpu
from test_gpu_attack import TAU, _attn_ref, agree_except_near_zero, f64, images, oracle_random_start, oracle_step, ref_grad, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
LN_EPS = 1e-6
U24 = 2.0 ** -24                 # half an ulp of 1 in fp32


def lib():
    from nested_diffusion_amd import _lib
    return _lib.load()


def check(rc, what):
    from nested_diffusion_amd import _lib
    _lib.check(rc, what)


def stream():
    return torch.cuda.current_stream().cuda_stream


def p(t):
    return None if t is None else t.data_ptr()


def poisoned(*shape):
    """fp32 GPU tensor whose every byte is 0xFF: a NaN in every element."""
    return torch.full((math.prod(shape) * 4,), 0xFF, dtype=torch.uint8, device=DEV).view(torch.float32).reshape(shape)


def image_buffer(rows, K, fill=0xFF):
    from nested_diffusion_amd import ops
    nbytes = lib().nd_split_bytes(rows, K)
    return ops.SplitMatrix(rows, K, DEV, data=torch.full((nbytes,), fill, dtype=torch.uint8, device=DEV))


def image_pieces(img, pad=False):
    """frag32b3 image -> its bf16 pieces as int16 [rows, K, 3] (csrc/nd_b9.hpp: 16 x 32 blocks of three 64-lane planes of 8 values,
    lane = row % 16 + 16 * (column % 32 / 8)).  The pad rows of the last block are dropped unless pad=True."""
    nrb, nkb = (img.rows + 15) // 16, img.K // 32
    t = img.data[: nrb * nkb * 3072].view(torch.int16).reshape(nrb, nkb, 3, 4, 16, 8)
    t = t.permute(0, 4, 1, 3, 5, 2).reshape(nrb * 16, img.K, 3)
    return t if pad else t[: img.rows]


def assert_image_is_split_of(img, out):
    """the image holds, bit for bit, the pieces nd_split_rows makes of the fp32 output (every valid row)."""
    from nested_diffusion_amd import ops
    assert torch.equal(image_pieces(img), image_pieces(ops.split_rows(out)))


def rel(a, b):
    """||a - b|| / ||b|| in float64 (a, b on any device)."""
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def within_fp32(err, err32, floor):
    """the fp32-relative rule: err_kernel <= max(floor, 4 * err_torch_fp32), both measured against float64."""
    return err <= max(floor, 4 * err32)


# ---- 1. attention_grad -------------------------------------------------------------------------------------------------------------
ATT_N = [1, 2, 15, 16, 17, 31, 33, 63, 64, 65, 128, 129, 192, 193, 197, 207, 208]
ATT_HEADS = [1, 3, 6, 12, 16]


def attention_inputs(B, N, heads, seed, qk_scale=1.0):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * N, 3 * heads * 64, generator=g)
    qkv[:, : 2 * heads * 64] *= qk_scale
    dout = torch.randn(B * N, heads * 64, generator=g)
    return qkv, dout


def attention_autograd(qkv, dout, B, N, heads, dtype):
    qq = qkv.to(dtype).requires_grad_(True)
    _attn_ref(qq, B, N, heads).backward(dout.to(dtype))
    return qq.grad


def attention_grad_abi(qkv, o, dout, B, N, heads, want_out=True, want_split=True):
    """nd_attention_bwd through the C ABI into poisoned outputs: (fp32 dqkv or None, image or None)."""
    E3 = 3 * heads * 64
    out = poisoned(B * N, E3) if want_out else None
    img = image_buffer(B * N, E3) if want_split else None
    check(lib().nd_attention_bwd(p(qkv), p(o), p(dout), p(out), p(img.data) if img else None, B, N, heads, stream()), "nd_attention_bwd")
    return out, img


def parts(dqkv, heads):
    E = heads * 64
    return {"dq": dqkv[:, :E], "dk": dqkv[:, E:2 * E], "dv": dqkv[:, 2 * E:]}


def run_attention_case(B, N, heads, seed):
    from nested_diffusion_amd import ops
    qkv, dout = attention_inputs(B, N, heads, seed)
    qkv_d, dout_d = qkv.to(DEV), dout.to(DEV)
    o = ops.attention(qkv_d, B, N, heads)
    ref = attention_autograd(qkv, dout, B, N, heads, torch.float64)
    out, img = attention_grad_abi(qkv_d, o, dout_d, B, N, heads)
    ref_parts = parts(ref, heads)
    for name, a in parts(out, heads).items():
        b = ref_parts[name]
        if float(b.norm()) == 0.0:
            # N = 1: a softmax over one key has no gradient; dq, dk are rounding residue only
            assert float(a.double().norm()) <= 1e-5 * float(ref.norm()), (name, B, N, heads)
        else:
            assert rel(a, b) <= 1e-5, (name, B, N, heads, rel(a, b))
    assert_image_is_split_of(img, out)
    out_only, _ = attention_grad_abi(qkv_d, o, dout_d, B, N, heads, want_split=False)
    _, img_only = attention_grad_abi(qkv_d, o, dout_d, B, N, heads, want_out=False)
    assert torch.equal(out_only, out)                                              # bitwise reproducible, with or without the image
    assert torch.equal(image_pieces(img_only), image_pieces(img))


@pytest.mark.parametrize("heads", ATT_HEADS)
@pytest.mark.parametrize("N", ATT_N)
def test_attention_grad_sweep(N, heads):
    """Query slices of 16 (a last slice of 1..15 rows), the seven 32-key dK / dV strides (keys 192..207: m = 6 only), phase 2's four
    64-lane key groups, phase 3b's split at (N + 1) / 2, up to the N <= 208 limit; B = 1 and 3."""
    for B in (1, 3):
        run_attention_case(B, N, heads, seed=1000 * N + 10 * heads + B)


def test_attention_grad_product_grid():
    """B * heads = 384 workgroups: the make_attacks batch of ViT-B/16."""
    run_attention_case(32, 197, 12, seed=7)


@pytest.mark.parametrize("N", [17, 64, 197, 208])
def test_attention_grad_peaked_softmax(N, record_property):
    """q and k scaled so that a row's scores spread over ~20: nearly one-hot probabilities, and dS = P (dP - delta) cancels, delta taken
    from the forward's O.  fp32-relative rule against torch's fp32 autograd."""
    from nested_diffusion_amd import ops
    B, heads = 2, 12
    qkv, dout = attention_inputs(B, N, heads, seed=N, qk_scale=2.0)
    q, k = qkv.reshape(B, N, 3, heads, 64).permute(2, 0, 3, 1, 4)[:2]
    s = (q @ k.transpose(-2, -1)) * 0.125
    assert float((s.amax(-1) - s.amin(-1)).median()) > 15 or N < 64           # the regime is reached
    qkv_d = qkv.to(DEV)
    o = ops.attention(qkv_d, B, N, heads)
    out, img = attention_grad_abi(qkv_d, o, dout.to(DEV), B, N, heads)
    ref = parts(attention_autograd(qkv, dout, B, N, heads, torch.float64), heads)
    t32 = parts(attention_autograd(qkv, dout, B, N, heads, torch.float32), heads)
    for name, a in parts(out, heads).items():
        err, err32 = rel(a, ref[name]), rel(t32[name], ref[name])
        record_property(f"{name}_err", err)
        record_property(f"{name}_err_torch32", err32)
        print(f"N={N} {name}: kernel {err:.3e}, torch fp32 {err32:.3e}")
        assert within_fp32(err, err32, 1e-5), (name, err, err32)
    assert_image_is_split_of(img, out)


# ---- 2. layernorm_grad -------------------------------------------------------------------------------------------------------------
LN_DIMS = [4, 36, 64, 128, 192, 256, 260, 384, 512, 768, 1024, 1028, 1280, 2048]


def layernorm_grad_abi(x, w, g, res, want_split):
    rows, dim = x.shape
    out = poisoned(rows, dim)
    img = image_buffer(rows, dim) if want_split else None
    check(lib().nd_layernorm_bwd(p(x), p(w), p(g), p(res), p(out), p(img.data) if img else None, rows, dim, LN_EPS, stream()),
          "nd_layernorm_bwd")
    return out, img


def layernorm_autograd(x, w, g, dtype):
    xx = x.to(dtype).requires_grad_(True)
    F.layer_norm(xx, (x.shape[1],), w.to(dtype), torch.zeros(x.shape[1], dtype=dtype), LN_EPS).backward(g.to(dtype))
    return xx.grad


@pytest.mark.parametrize("dim", LN_DIMS)
@pytest.mark.parametrize("rows", [1, 3, 17, 591])
def test_layernorm_grad_sweep(rows, dim):
    """Every instantiation k_layernorm_bwd<1, 2, 3, 4, 8>, the dims just past each boundary, dims that are no multiple of 32 (fp32
    output only); with and without the residual; rows off the 4-rows-per-workgroup grid."""
    g = torch.Generator().manual_seed(rows * 10000 + dim)
    x = torch.randn(rows, dim, generator=g) * 2 + 0.3
    w = 1 + 0.1 * torch.randn(dim, generator=g)
    dy = torch.randn(rows, dim, generator=g)
    res = torch.randn(rows, dim, generator=g)
    ref = layernorm_autograd(x, w, dy, torch.float64)
    split = dim % 32 == 0
    for r in (None, res):
        out, img = layernorm_grad_abi(x.to(DEV), w.to(DEV), dy.to(DEV), r.to(DEV) if r is not None else None, split)
        got = out.cpu().double() - (r.double() if r is not None else 0)
        assert rel(got, ref) <= 1e-5, (rows, dim, r is not None, rel(got, ref))
        if split:
            assert_image_is_split_of(img, out)


@pytest.mark.parametrize("dim", [36, 768, 2048])
def test_layernorm_grad_edge_rows(dim, record_property):
    """A constant row (rstd = 1 / sqrt(eps)), a row of mean 1e3 and spread 1e-2, a row whose incoming gradient is zero; fp32-relative
    rule per row."""
    g = torch.Generator().manual_seed(dim)
    x = torch.randn(4, dim, generator=g)
    x[0] = 0.7
    x[1] = 1e3 + 1e-2 * torch.randn(dim, generator=g)
    w = 1 + 0.1 * torch.randn(dim, generator=g)
    dy = torch.randn(4, dim, generator=g)
    dy[2] = 0
    ref = layernorm_autograd(x, w, dy, torch.float64)
    t32 = layernorm_autograd(x, w, dy, torch.float32)
    out, _ = layernorm_grad_abi(x.to(DEV), w.to(DEV), dy.to(DEV), None, False)
    out = out.cpu()
    for r, what in ((0, "constant"), (1, "mean 1e3"), (3, "random")):
        err, err32 = rel(out[r], ref[r]), rel(t32[r], ref[r])
        record_property(f"{what}_err", err)
        record_property(f"{what}_err_torch32", err32)
        print(f"dim={dim} {what} row: kernel {err:.3e}, torch fp32 {err32:.3e}")
        assert within_fp32(err, err32, 1e-5), (what, err, err32)
    assert torch.equal(out[2], torch.zeros(dim))                                  # g = 0: exactly zero


# ---- 3. xent_head_grad -------------------------------------------------------------------------------------------------------------
def xent_head_grad_abi(logits, labels, w):
    B, C = logits.shape
    E = w.shape[1]
    dfeat, loss = poisoned(B, E), poisoned(B)
    check(lib().nd_xent_head_bwd(p(logits), p(labels), p(w), p(dfeat), p(loss), B, C, E, stream()), "nd_xent_head_bwd")
    return dfeat.cpu(), loss.cpu()


@pytest.mark.parametrize("E", [1, 3, 192, 1025])
@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 256, 257, 1000, 1024])
def test_xent_head_grad_sweep(C, E):
    """One wave reduces over C (C > 64: several values per lane), a 256-thread loop writes the C values of d (C <= 1024, the LDS
    array), a 256-thread loop over E; B = 1 and 33.  d = p - 1 at the label cancels in fp32 when p_y is near 1: fp32-relative rule
    against torch's fp32 autograd for dfeat."""
    for B in (1, 33):
        g = torch.Generator().manual_seed(C * 10000 + E * 10 + B)
        logits = torch.randn(B, C, generator=g) * 3
        labels = torch.randint(0, C, (B,), generator=g)
        w = torch.randn(C, E, generator=g)
        ll = logits.double().requires_grad_(True)
        loss64 = F.cross_entropy(ll, labels, reduction="none")
        loss64.sum().backward()
        l32 = logits.clone().requires_grad_(True)
        F.cross_entropy(l32, labels, reduction="sum").backward()
        dfeat, loss = xent_head_grad_abi(logits.to(DEV), labels.to(DEV), w.to(DEV))
        if C == 1:                                                                # softmax of one class: no gradient, no loss
            assert torch.equal(dfeat, torch.zeros(B, E)) and torch.equal(loss, torch.zeros(B))
            continue
        ref = ll.grad @ w.double()
        err, err32 = rel(dfeat, ref), rel(l32.grad @ w, ref)
        assert within_fp32(err, err32, 1e-5), (B, C, E, err, err32)
        bound = 4 * U24 * logits.double().abs().max(1).values.clamp(min=1)       # the rounding of logsumexp at the max logit's scale
        assert bool(((loss.double() - loss64.detach()).abs() <= bound).all()), (B, C, E)


@pytest.mark.parametrize("C", [2, 10, 1000])
@pytest.mark.parametrize("margin", [0, 5, 15, 20, 40, 90, 110])
def test_xent_head_grad_confident_logits(margin, C, record_property):
    """A trained head's large margins.  Half the rows lead with the label by `margin`, half are confidently wrong (another class leads the
    label by `margin`).  Where 1 - p_y drops below fp32's resolution, softmax - onehot rounds to 0 at the label, as in torch's fp32 (and in
    the foolbox loop the reference runs): pinned here.  With head_w = I the kernel's d = softmax - onehot is read out exactly."""
    B = 16
    g = torch.Generator().manual_seed(margin * 100 + C)
    logits = 8 + 0.5 * torch.randn(B, C, generator=g)                            # an offset: the loss bar scales with |max logit|
    labels = torch.randint(0, C, (B,), generator=g)
    rows = torch.arange(B)
    lead = logits.max(1).values + margin
    logits[rows[: B // 2], labels[: B // 2]] = lead[: B // 2]
    other = (labels[B // 2:] + 1) % C
    logits[rows[B // 2:], other] = logits[rows[B // 2:], labels[B // 2:]] + margin
    onehot = F.one_hot(labels, C)
    d32 = torch.softmax(logits, 1) - onehot                                      # torch fp32
    l64 = logits.double()
    d64 = torch.softmax(l64, 1) - onehot
    one_minus_py = 1 - torch.softmax(l64, 1)[rows, labels]
    eye = torch.eye(C)
    d, loss = xent_head_grad_abi(logits.to(DEV), labels.to(DEV), eye.to(DEV))
    d = d.double()
    # against the fp32 softmax, element by element: p = exp(l - max) / sum differs by the rounding of a C-term sum (one wave: C / 64
    # terms per lane, then 6 butterfly steps; torch sums in another order), a few ulps of p -- of 1 at the label -- or a denormal
    p32 = torch.softmax(logits, 1).double()
    ulps = 2 * (math.ceil(C / 64) + 8) * U24 * (p32 + onehot) + 2.0 ** -126
    assert bool(((d - d32.double()).abs() <= ulps).all()), float(((d - d32.double()).abs() / p32).max())
    # against true float64 where fp32 can resolve 1 - p_y: fp32-relative rule row by row
    for b in range(B):
        if float(one_minus_py[b]) > 2.0 ** -20:
            err, err32 = rel(d[b], d64[b]), rel(d32[b], d64[b])
            assert within_fp32(err, err32, 1e-5), (b, err, err32)
    # the pinned rounding: 1 - p_y below half an ulp of 1 gives exactly 0 at the label, in the kernel as in torch's fp32
    gone = one_minus_py < 2.0 ** -25
    assert torch.equal(d[rows, labels][gone], torch.zeros(int(gone.sum()), dtype=torch.float64))
    assert torch.equal(d32[rows, labels][gone], torch.zeros(int(gone.sum())))
    record_property("rows_rounded_to_zero", int(gone.sum()))
    # a dense head: dfeat = d . W against float64 of the fp32 softmax times W
    E = 64
    w = torch.randn(C, E, generator=g)
    dfeat, _ = xent_head_grad_abi(logits.to(DEV), labels.to(DEV), w.to(DEV))
    want = d32.double() @ w.double()
    scale = d32.double().abs() @ w.double().abs()
    tol = ulps @ w.double().abs() + (C + 4) * U24 * scale
    assert bool(((dfeat.double() - want).abs() <= tol).all())
    # the loss against float64 log-sum-exp
    want_loss = torch.logsumexp(l64, 1) - l64[rows, labels]
    bound = 4 * U24 * l64.abs().max(1).values.clamp(min=1)
    assert bool(((loss.double() - want_loss).abs() <= bound).all()), float((loss.double() - want_loss).abs().max())


# ---- 4. GELU images ------------------------------------------------------------------------------------------------------------------
EDGE_ARGS = [0.0, -0.0, 1e-30, -1e-30, 30.0, -30.0, 1e4, -1e4]


@pytest.mark.parametrize("rows", [1, 15, 17])
def test_gelu_images_at_edge_arguments(rows):
    """nd_gelu_split / nd_gelu_bwd_split at 0, -0, +-1e-30, +-30, +-1e4 (element by element against float64) among random values (rel
    L2), the image is the split of the fp32 output, and the pad rows of the last 16-row block are written as zeros."""
    cols, n_edge = 32, len(EDGE_ARGS) * 3
    g = torch.Generator().manual_seed(rows)
    u = torch.randn(rows, cols, generator=g) * 3
    u.view(-1)[:n_edge] = torch.tensor(EDGE_ARGS * 3)
    dg = torch.randn(rows, cols, generator=g)
    uu = u.double().requires_grad_(True)
    y64 = F.gelu(uu)
    y64.backward(dg.double())
    ud, dgd = u.to(DEV), dg.to(DEV)
    for bwd, ref in ((False, y64.detach()), (True, uu.grad)):
        out, img = poisoned(rows, cols), image_buffer(rows, cols)
        if bwd:
            rc = lib().nd_gelu_bwd_split(p(ud), p(dgd), p(out), p(img.data), rows, cols, stream())
        else:
            rc = lib().nd_gelu_split(p(ud), p(out), p(img.data), rows, cols, stream())
        check(rc, "nd_gelu_split")
        got = out.cpu().double()
        e_got, e_ref = got.view(-1)[:n_edge], ref.view(-1)[:n_edge]
        assert bool(((e_got - e_ref).abs() <= 2e-6 * e_ref.abs() + 1e-37).all()), (bwd, e_got, e_ref)
        assert rel(got, ref) <= 1e-5, bwd
        assert_image_is_split_of(img, out)
        assert bool((image_pieces(img, pad=True)[rows:] == 0).all())


# ---- 5. poisoned pad rows ahead of the dX GEMM -------------------------------------------------------------------------------------
def test_pad_rows_of_the_backward_images_do_not_reach_the_dx_gemm():
    """nd_layernorm_bwd and nd_attention_bwd never write the pad rows of their image's last 16-row block; the next gemm_split of
    _block_grad reads that image as its A operand.  With B * N = 3 * 197 rows, a buffer of 0xFF bytes (bf16 NaNs) and a zeroed one
    must give the same GEMM result, bit for bit."""
    from nested_diffusion_amd import ops
    B, N, heads = 3, 197, 12
    E, rows = heads * 64, 3 * 197
    g = torch.Generator().manual_seed(55)
    x = (torch.randn(rows, E, generator=g) * 2).to(DEV)
    w = (1 + 0.1 * torch.randn(E, generator=g)).to(DEV)
    dy = torch.randn(rows, E, generator=g).to(DEV)
    res = torch.randn(rows, E, generator=g).to(DEV)
    qkv = torch.randn(rows, 3 * E, generator=g).to(DEV)
    o = ops.attention(qkv, B, N, heads)
    wT_proj = ops.split_rows((torch.randn(E, E, generator=g) / E ** 0.5).to(DEV))
    wT_qkv = ops.split_rows((torch.randn(E, 3 * E, generator=g) / E ** 0.5).to(DEV))
    results = {}
    for fill in (0xFF, 0x00):
        ln = image_buffer(rows, E, fill)
        check(lib().nd_layernorm_bwd(p(x), p(w), p(dy), p(res), None, p(ln.data), rows, E, LN_EPS, stream()), "nd_layernorm_bwd")
        att = image_buffer(rows, 3 * E, fill)
        check(lib().nd_attention_bwd(p(qkv), p(o), p(dy), None, p(att.data), B, N, heads, stream()), "nd_attention_bwd")
        if fill == 0xFF:
            assert bool((image_pieces(ln, pad=True)[rows:] == -1).all()) and bool((image_pieces(att, pad=True)[rows:] == -1).all())
        results[fill] = (ops.gemm_split(ln, wT_proj), ops.gemm_split(att, wT_qkv))
    for a, b in zip(results[0xFF], results[0x00]):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b)


# ---- 6. Linf kernels at the product size ---------------------------------------------------------------------------------------------
def host_linf_step(x, x0, g, alpha, eps, lo, hi):
    """nd_linf_step restated in numpy float32, one rounding per operation; sign(0) = sign(-0) = 0 and a NaN gradient is no step."""
    f = np.float32
    s = np.zeros_like(x) if g is None else np.where(g > 0, f(1), np.where(g < 0, f(-1), f(0))).astype(np.float32)
    step = x + f(alpha) * s
    d = np.minimum(np.maximum(step - x0, -f(eps)), f(eps))
    return np.minimum(np.maximum(x0 + d, f(lo)), f(hi))


def linf_step_abi(x, x0, g, alpha, eps, lo, hi):
    out = poisoned(x.numel())
    check(lib().nd_linf_step(p(x), p(x0), p(g), p(out), x.numel(), alpha, eps, lo, hi, stream()), "nd_linf_step")
    return out


@pytest.mark.parametrize("n", [32 * 3 * 224 * 224, 2097153])
def test_linf_step_bitwise_at_the_product_size(n):
    """n = 32 x 3 x 224^2 (the make_attacks batch: three passes of the 8192 x 256 grid) and one element past a single pass.  Gradient
    entries 0, -0, +-denormal, +-inf and NaN everywhere in the array, x and x0 at both bounds, eps = 0, alpha > eps, no gradient with
    infinite bounds: every element bit for bit against the float32 restatement."""
    rng = np.random.default_rng(n)
    eps0 = np.float32(8 / 255)
    x0 = rng.random(n, dtype=np.float32)
    x = np.clip(x0 + rng.uniform(-2 * eps0, 2 * eps0, n).astype(np.float32), 0, 1).astype(np.float32)
    g = rng.standard_normal(n, dtype=np.float32)
    for k, v in enumerate([0.0, -0.0, 1e-40, -1e-40, np.inf, -np.inf, np.nan]):
        g[k::101] = v
    x[::13], x[5::13], x0[3::17], x0[7::17] = 0, 1, 0, 1
    xd, x0d, gd = (torch.from_numpy(a).to(DEV) for a in (x, x0, g))
    inf = float("inf")
    cases = [(8 / 255, 8 / 255, 0.0, 1.0, True), (0.01 / 0.3 * 8 / 255, 8 / 255, 0.0, 1.0, True), (0.01, 0.0, 0.0, 1.0, True),
             (0.1, 0.03, 0.0, 1.0, True), (0.0, 8 / 255, -inf, inf, False)]
    for alpha, eps, lo, hi, with_grad in cases:
        out = linf_step_abi(xd, x0d, gd if with_grad else None, alpha, eps, lo, hi).cpu().numpy()
        want = host_linf_step(x, x0, g if with_grad else None, alpha, eps, lo, hi)
        bad = np.flatnonzero(out.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, (alpha, eps, lo, hi, with_grad, bad[:8], bad.size)
    # a NaN gradient is no step (torch.sign would make it NaN)
    nan_at = np.flatnonzero(np.isnan(g))[-1]
    out = linf_step_abi(xd, x0d, gd, 8 / 255, 8 / 255, 0.0, 1.0)
    assert float(out[nan_at]) == float(np.clip(x0[nan_at] + np.clip(x[nan_at] - x0[nan_at], -eps0, eps0), 0, 1))


def test_linf_random_start_at_the_product_size():
    """B = 32 at 224^2 against the Philox restatement; restart != 0; first_image = 2^32 - 3, whose counter wraps inside the batch; a
    sub-batch keyed at its offset draws the rows of the whole batch."""
    from nested_diffusion_amd import ops
    x0 = images(32, 224, 61)
    xd = x0.to(DEV)
    eps, seed = 8 / 255, 0xDEAD_BEEF_1234
    for first, restart in ((0, 0), (1000, 3), (2 ** 32 - 3, 1)):
        s = ops.linf_random_start(xd, eps, seed, first_image=first, restart=restart)
        assert torch.equal(s.cpu(), oracle_random_start(x0, eps, seed, first, restart)), (first, restart)
        sub = ops.linf_random_start(xd[2:7].contiguous(), eps, seed, first_image=(first + 2) % 2 ** 32, restart=restart)
        assert torch.equal(sub, s[2:7])
    a = ops.linf_random_start(xd, eps, seed, 0, 0)
    assert not torch.equal(a, ops.linf_random_start(xd, eps, seed, 0, 1))       # restarts draw afresh


@pytest.mark.parametrize("B,Cin,H,W,patch", [(2, 1, 32, 48, 4), (3, 3, 64, 40, 8), (2, 3, 224, 224, 16), (1, 1, 96, 160, 32),
                                             (2, 3, 64, 96, 32), (70, 3, 224, 224, 16)])
def test_unpatchify_is_the_inverse_permutation(B, Cin, H, W, patch):
    """p = 4, 8, 16, 32; one and three channels; non-square images; B = 70 at 224^2 runs the grid-stride loop.  Equal to the inverse
    permutation written with reshape / permute, and the adjoint of patchify: <patchify(x), y> = <x, unpatchify(y)>."""
    from nested_diffusion_amd import ops
    g = torch.Generator().manual_seed(B * 1000 + patch)
    gh, gw = H // patch, W // patch
    cols = torch.randn(B * gh * gw, Cin * patch * patch, generator=g)
    cols_d, img = cols.to(DEV), poisoned(B, Cin, H, W)
    check(lib().nd_unpatchify(p(cols_d), p(img), B, Cin, H, W, patch, stream()), "nd_unpatchify")
    want = cols.reshape(B, gh, gw, Cin, patch, patch).permute(0, 3, 1, 4, 2, 5).reshape(B, Cin, H, W)
    assert torch.equal(img.cpu(), want)
    x = torch.randn(B, Cin, H, W, generator=g)
    lhs = float((ops.patchify(x.to(DEV), patch).cpu().double() * cols.double()).sum())
    rhs = float((x.double() * img.cpu().double()).sum())
    assert math.isclose(lhs, rhs, rel_tol=1e-12, abs_tol=1e-9)


# ---- 7. input_grad at the product shape and at other geometries ------------------------------------------------------------------
def check_input_grad(vit, vp, heads, depth, x, labels):
    """input_grad against the oracle in float64: (rel L2, max-rel) of the gradient; asserts the logits are forward()'s."""
    logits, dx, loss = vit.input_grad(x.to(DEV), labels.to(DEV))
    assert torch.equal(logits, vit.forward(x.to(DEV)))
    ref_logits, g_ref = ref_grad(f64(vp), x, labels, heads, depth)
    assert rel_l2(loss, F.cross_entropy(ref_logits, labels, reduction="none")) <= 1e-5
    return dx, g_ref, rel_l2(dx, g_ref), float((dx.cpu().double() - g_ref).abs().max() / g_ref.abs().max())


@pytest.fixture(scope="module")
def vitb_b32():
    """ViT-B/16 with the make_attacks batch of 32 images at 224^2, and its float64 input gradient (computed once)."""
    from nested_diffusion_amd.mapping import VisionTransformer
    vp = ref_cpu.init_vit_params(embed=768, depth=12, patch=16, img=224, seed=13)
    vit = VisionTransformer(vp, 12, DEV)
    x = images(32, 224, 71)
    labels = torch.arange(32) % 2
    _, g_ref = ref_grad(f64(vp), x, labels, 12, 12)
    return vit, vp, x, labels, g_ref


def test_input_grad_at_the_make_attacks_batch(vitb_b32, record_property):
    vit, vp, x, labels, g_ref = vitb_b32
    logits, dx, loss = vit.input_grad(x.to(DEV), labels.to(DEV))
    assert torch.equal(logits, vit.forward(x.to(DEV)))
    r, m = rel_l2(dx, g_ref), float((dx.cpu().double() - g_ref).abs().max() / g_ref.abs().max())
    record_property("grad_rel_l2", r)
    record_property("grad_max_rel", m)
    print(f"ViT-B/16 B=32: input gradient rel L2 {r:.3e}, max-rel {m:.3e}")
    assert r <= 1e-4 and m <= TAU
    _, dx2, loss2 = vit.input_grad(x.to(DEV), labels.to(DEV))
    assert torch.equal(dx2, dx) and torch.equal(loss2, loss)                     # run to run, bit for bit


def test_fgsm_at_the_make_attacks_batch(vitb_b32):
    from nested_diffusion_amd.attack import Attack
    vit, vp, x, labels, g_ref = vitb_b32
    eps = 8 / 255
    adv, _ = Attack(eps, "FGSM", vit).generate_attack(x.to(DEV), labels.to(DEV))
    ok, frac = agree_except_near_zero(adv, oracle_step(x, x, g_ref, eps, eps), g_ref)
    assert ok and frac > 0.9


GEOMETRIES = {                                   # embed, patch, img, depth, B
    "vit_b32": (768, 32, 224, 4, 2),             # N = 50
    "vit_s16": (384, 16, 224, 4, 2),             # 6 heads
    "vit_ti16": (192, 16, 224, 4, 5),            # 3 heads
    "wide_1024": (1024, 16, 224, 2, 1),          # 16 heads, LayerNorm backward <4>
    "img208": (768, 16, 208, 2, 1),              # N = 170
}


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_input_grad_other_geometries(name, record_property):
    from nested_diffusion_amd.mapping import VisionTransformer
    embed, patch, img, depth, B = GEOMETRIES[name]
    heads = embed // 64
    vp = ref_cpu.init_vit_params(embed=embed, depth=depth, patch=patch, img=img, seed=len(name))
    vit = VisionTransformer(vp, heads, DEV)
    x = images(B, img, 81)
    labels = torch.arange(B) % 2
    _, _, r, m = check_input_grad(vit, vp, heads, depth, x, labels)
    record_property("grad_rel_l2", r)
    record_property("grad_max_rel", m)
    assert r <= 1e-4 and m <= TAU, (r, m)


def test_input_grad_trained_like_vit(record_property):
    """ViT-B/16 at depth 4 with q / k weights scaled for peaked attention and the head for logit margins of about 10: fp32-relative
    rule against the oracle run by torch in fp32."""
    from nested_diffusion_amd.mapping import VisionTransformer
    depth, E = 4, 768
    vp = ref_cpu.init_vit_params(embed=E, depth=depth, patch=16, img=224, seed=17)
    for i in range(depth):
        vp[f"blocks.{i}.attn.qkv.weight"][: 2 * E] *= 2.0
    vp["head.weight"] *= 3.0
    vit = VisionTransformer(vp, 12, DEV)
    x = images(4, 224, 91)
    logits32 = ref_cpu.vit_full_forward(vp, x, 12, depth)
    labels = torch.tensor([0, 1, 1, 0])
    dx, g_ref, r, m = check_input_grad(vit, vp, 12, depth, x, labels)
    xx = x.clone().requires_grad_(True)
    F.cross_entropy(ref_cpu.vit_full_forward(vp, xx, 12, depth), labels, reduction="sum").backward()
    r32 = rel_l2(xx.grad, g_ref)
    m32 = float((xx.grad.double() - g_ref).abs().max() / g_ref.abs().max())
    margin = float((logits32[:, 0] - logits32[:, 1]).abs().min())
    for k, v in (("margin", margin), ("grad_rel_l2", r), ("grad_max_rel", m), ("torch32_rel_l2", r32), ("torch32_max_rel", m32)):
        record_property(k, v)
    print(f"trained-like ViT-B: margin >= {margin:.1f}; kernel {r:.3e} / {m:.3e}, torch fp32 {r32:.3e} / {m32:.3e}")
    assert margin > 5
    assert within_fp32(r, r32, 1e-4) and within_fp32(m, m32, TAU)


@pytest.mark.parametrize("att_f32", [False, True])
def test_input_grad_with_and_without_the_attention_images(att_f32, monkeypatch):
    """A geometry whose token count allows the bf16-pipe attention of the forward (3 x 5 patches + cls = 16 tokens); ND_ATT_F32=1
    switches it to the fp32 attention.  Either way the logits are forward()'s under the same setting and the gradient meets the bars."""
    from nested_diffusion_amd import ops
    from nested_diffusion_amd.mapping import VisionTransformer
    if att_f32:
        monkeypatch.setenv("ND_ATT_F32", "1")
    else:
        monkeypatch.delenv("ND_ATT_F32", raising=False)
    E, depth = 768, 2
    vp = ref_cpu.init_vit_params(embed=E, depth=depth, patch=16, img=48, seed=23)
    vp["pos_embed"] = torch.randn(1, 16, E, generator=torch.Generator().manual_seed(24)) * 0.02
    vit = VisionTransformer(vp, 12, DEV)
    assert ops.qkv_images_supported(16, 12)
    x = torch.rand(3, 3, 48, 80, generator=torch.Generator().manual_seed(25))
    _, _, r, m = check_input_grad(vit, vp, 12, depth, x, torch.tensor([0, 1, 1]))
    assert r <= 1e-4 and m <= TAU, (r, m)


def test_input_grad_at_the_token_limit():
    """9 x 23 patches + cls = 208 tokens, the attention backward's limit."""
    from nested_diffusion_amd.mapping import VisionTransformer
    vp = ref_cpu.init_vit_params(embed=128, depth=2, patch=16, img=16, seed=29)
    vp["pos_embed"] = torch.randn(1, 208, 128, generator=torch.Generator().manual_seed(30)) * 0.02
    vit = VisionTransformer(vp, 2, DEV)
    x = torch.rand(2, 3, 144, 368, generator=torch.Generator().manual_seed(31))
    _, _, r, m = check_input_grad(vit, vp, 2, 2, x, torch.tensor([1, 0]))
    assert r <= 1e-4 and m <= TAU, (r, m)


def test_input_grad_refuses_too_many_tokens_before_the_forward(monkeypatch):
    """240 x 240 at patch 16: 226 tokens.  The limit is named, and nothing has run on the GPU when the error is raised."""
    from nested_diffusion_amd import _lib
    from nested_diffusion_amd.mapping import VisionTransformer
    vp = ref_cpu.init_vit_params(embed=128, depth=1, patch=16, img=240, seed=37)
    vit = VisionTransformer(vp, 2, DEV)

    def must_not_run(*a, **k):
        raise AssertionError("the forward ran before the token limit was checked")
    monkeypatch.setattr(vit, "_tokens", must_not_run)
    monkeypatch.setattr(vit, "transposed_weights", must_not_run)
    with pytest.raises(_lib.NdError, match=r"N <= 208.*N=226"):
        vit.input_grad(torch.rand(1, 3, 240, 240).to(DEV), torch.tensor([0]).to(DEV))
