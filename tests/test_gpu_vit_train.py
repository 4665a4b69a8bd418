"""Training of the ViT on the GPU: nd_gemm_tn_adamw (the weight gradient of a thousands-of-rows contraction on the matrix pipe, AdamW applied
to the row-major weight in registers), nd_colsum_adamw, nd_layernorm_wgrad_adamw, and ViTTrainer end to end against float64 autograd
through the CPU oracle."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_cpu
from test_vit_train_host import adamw_f32, chunked_colsum_f32

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
LN_EPS = 1e-6


def gen(seed):
    return torch.Generator().manual_seed(seed)


def plan_shape(which):
    """(M, N, K) from the kernel's own plan.  'ragged': the last tiles over N and over K are partly filled (and there is more than one
    tile each way); 'mtile': M is one past a multiple of the rows per LDS stage."""
    from nested_diffusion_amd import ops
    p = ops.gemm_tn_plan(16, 16)
    if which == "ragged":
        M, N, K = 15, p["tile_n"] + 17, p["tile_k"] + 16
        q = ops.gemm_tn_plan(N, K)
        assert q["grid_n"] == 2 and q["grid_k"] == 2 and N % q["tile_n"] and K % q["tile_k"]
        return M, N, K
    return 2 * p["m_tile"] + 1, 33, 48


def rel_l2(got, ref):
    got, ref = got.double().flatten(), ref.double().flatten()
    return float((got - ref).norm() / ref.norm())


# ---- 1. the GEMM gradient -------------------------------------------------------------------------------------------------------------
GRAD_SHAPES = [(1, 1, 16), (3, 2, 16), (15, 2, 128), (15, 17, 48), (394, 33, 304), "ragged", "mtile", (5910, 768, 768)]


@pytest.mark.parametrize("shape", GRAD_SHAPES, ids=str)
def test_gemm_gradient_is_within_the_rounding_bound(shape):
    """(M + 2) 2^-24 sum_m |dy x| |gscale| per element: one rounding per product, M - 1 sums, one scale"""
    from nested_diffusion_amd import ops
    M, N, K = plan_shape(shape) if isinstance(shape, str) else shape
    g = gen(M * 1000 + N)
    dy, x, gscale = torch.randn(M, N, generator=g), torch.randn(M, K, generator=g), 1.0 / 3.0
    got = ops.gemm_tn_adamw(dy.to(DEV), x.to(DEV), None, None, None, None, gscale=gscale, return_grad=True)
    assert tuple(got.shape) == (N, K)
    got = got.cpu().double()
    ref = dy.double().t() @ x.double() * float(np.float32(gscale))
    bound = (M + 2) * U * (dy.double().abs().t() @ x.double().abs()) * float(np.float32(gscale))
    excess = ((got - ref).abs() - bound).max()
    print(f"{(M, N, K)}: max |g - g64| = {float((got - ref).abs().max()):.3e}, max bound = {float(bound.max()):.3e}")
    assert float(excess) <= 0.0, (M, N, K, float(excess))
    # the same bits on a second run, and w / m / v untouched by a gradient-only call that is handed them
    w, m, v = (torch.full((N, K), c, device=DEV) for c in (1.0, 2.0, 3.0))
    lib_g, dyd, xd = torch.empty(N, K, device=DEV), dy.to(DEV), x.to(DEV)
    from nested_diffusion_amd import _lib
    _lib.check(_lib.load().nd_gemm_tn_adamw(_lib.ptr(dyd), _lib.ptr(xd), _lib.ptr(w), _lib.ptr(m), _lib.ptr(v), _lib.ptr(lib_g), M, N, K, gscale,
                                            None, ops._stream(dyd)), "nd_gemm_tn_adamw")
    torch.cuda.synchronize()
    assert torch.equal(lib_g.cpu().double(), got)
    assert bool((w == 1.0).all()) and bool((m == 2.0).all()) and bool((v == 3.0).all())


# ---- 2. the fused GEMM update, bit for bit --------------------------------------------------------------------------------------------
def _state(shape, with_state, g):
    w0 = torch.randn(*shape, generator=g) * 0.1
    m0 = torch.randn(*shape, generator=g) * 0.05 if with_state else torch.zeros(*shape)
    v0 = torch.rand(*shape, generator=g) * 0.01 if with_state else torch.zeros(*shape)
    return w0, m0, v0


def _check_update(w, m, v, w0, m0, v0, G, a, lr):
    we, me, ve = adamw_f32(w0.numpy(), m0.numpy(), v0.numpy(), G, a)
    np.testing.assert_array_equal(m.cpu().numpy(), me)
    np.testing.assert_array_equal(v.cpu().numpy(), ve)
    np.testing.assert_array_equal(w.cpu().numpy(), we)
    if lr == 0.0:
        assert a.decay == 1.0 and np.array_equal(w.cpu().numpy().view(np.uint32), w0.numpy().view(np.uint32))
    else:
        assert not np.array_equal(we, w0.numpy())


@pytest.mark.parametrize("M,N,K", [(3, 2, 16), (15, 17, 48), (394, 33, 304)])
@pytest.mark.parametrize("t,lr,with_state", [(1, 1e-4, False), (7, 1e-4, True), (7, 0.0, True)])
def test_gemm_update_equals_the_float32_listing_bit_for_bit(M, N, K, t, lr, with_state):
    from nested_diffusion_amd import ops
    g = gen(100 * t + N)
    dy, x = torch.randn(M, N, generator=g), torch.randn(M, K, generator=g)
    w0, m0, v0 = _state((N, K), with_state, g)
    w, m, v = w0.to(DEV), m0.to(DEV), v0.to(DEV)
    ptrs = (w.data_ptr(), m.data_ptr(), v.data_ptr())
    a = ops.adamw_step(lr, t)
    G = ops.gemm_tn_adamw(dy.to(DEV), x.to(DEV), w, m, v, a, gscale=1.0 / M, return_grad=True).cpu().numpy()
    only = ops.gemm_tn_adamw(dy.to(DEV), x.to(DEV), None, None, None, None, gscale=1.0 / M, return_grad=True).cpu().numpy()
    np.testing.assert_array_equal(G, only)                    # the fused call forms the gradient-only call's gradient
    _check_update(w, m, v, w0, m0, v0, G, a, lr)
    assert ptrs == (w.data_ptr(), m.data_ptr(), v.data_ptr())
    # without g_out: the same update
    w2, m2, v2 = w0.to(DEV), m0.to(DEV), v0.to(DEV)
    assert ops.gemm_tn_adamw(dy.to(DEV), x.to(DEV), w2, m2, v2, a, gscale=1.0 / M) is None
    assert torch.equal(w2, w) and torch.equal(m2, m) and torch.equal(v2, v)


# ---- 3. the column sum ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 15, "chunk", "chunk+1", "2chunk", "2chunk+1", 5910], ids=str)
def test_colsum_is_the_documented_order_bit_for_bit(M):
    """(above two chunks of rows the kernel runs in its narrow form, 16 columns a workgroup: both sides of that threshold are cases)"""
    from nested_diffusion_amd import ops
    chunk = ops.COLSUM_CHUNK
    M = {"chunk": chunk, "chunk+1": chunk + 1, "2chunk": 2 * chunk, "2chunk+1": 2 * chunk + 1}.get(M, M)
    N = 70                                                    # two workgroups of columns, the second partly filled
    dy = torch.randn(M, N, generator=gen(3 + M))
    if M >= 15:
        # columns whose float32 sum depends on the order: a large term, small ones it swallows, and its cancellation
        dy[:, 0] = 1.0
        dy[0, 0], dy[M - 2, 0] = 2.0 ** 25, -2.0 ** 25
        dy[:, 69] = torch.tensor(([1e8, 1.0, -1e8, 1.0] * M)[:M])
    want = chunked_colsum_f32(dy.numpy(), chunk)
    if M >= 15:
        rev = np.zeros(N, np.float32)
        for r in reversed(range(M)):
            rev = rev + dy[r].numpy()
        assert want[0] != rev[0] and want[0] != np.float32(dy[:, 0].double().sum())
    if M > 2 * chunk:                                         # the chunked order is not the plain row order either
        plain = np.zeros(N, np.float32)
        for r in range(M):
            plain = plain + dy[r].numpy()
        assert not np.array_equal(plain, want)
    gscale = np.float32(1.0 / 3.0)
    G = want * gscale
    only = ops.colsum_adamw(dy.to(DEV), None, None, None, None, gscale=1.0 / 3.0, return_grad=True)
    np.testing.assert_array_equal(only.cpu().numpy(), G)
    for t, lr, with_state in ((1, 1e-4, False), (7, 1e-4, True), (7, 0.0, True)):
        b0, m0, v0 = _state((N,), with_state, gen(t))
        b, m, v = b0.to(DEV), m0.to(DEV), v0.to(DEV)
        a = ops.adamw_step(lr, t)
        got = ops.colsum_adamw(dy.to(DEV), b, m, v, a, gscale=1.0 / 3.0, return_grad=True)
        np.testing.assert_array_equal(got.cpu().numpy(), G)
        _check_update(b, m, v, b0, m0, v0, G, a, lr)


def test_colsum_does_not_depend_on_the_width():
    """the order is a function of M alone: a column gives the same bits alone, among 70 and among 1000 columns"""
    from nested_diffusion_amd import ops
    M = 3 * ops.COLSUM_CHUNK + 5
    dy = torch.randn(M, 1000, generator=gen(8)).to(DEV)
    wide = ops.colsum_adamw(dy, None, None, None, None, return_grad=True)
    for lo, hi in ((0, 1), (999, 1000), (3, 73)):
        part = ops.colsum_adamw(dy[:, lo:hi].contiguous(), None, None, None, None, return_grad=True)
        assert torch.equal(part, wide[lo:hi])


# ---- 4. the LayerNorm parameter gradient ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,dim", [(1, 128), (15, 128), (394, 768)])
def test_layernorm_parameter_gradient(rows, dim):
    from nested_diffusion_amd import ops
    g = gen(rows + dim)
    x = torch.randn(rows, dim, generator=g) * 1.5 + 0.3
    dyo = torch.randn(rows, dim, generator=g)
    gamma0, beta0 = 1.0 + 0.1 * torch.randn(dim, generator=g), 0.05 * torch.randn(dim, generator=g)
    ga, be = gamma0.double().requires_grad_(), beta0.double().requires_grad_()
    (F.layer_norm(x.double(), (dim,), ga, be, LN_EPS) * dyo.double()).sum().backward()
    gscale = 0.25
    dg, db = ops.layernorm_wgrad_adamw(x.to(DEV), dyo.to(DEV), LN_EPS, None, None, None, None, None, None, None, gscale=gscale, return_grad=True)
    eg, eb = rel_l2(dg.cpu(), ga.grad * gscale), rel_l2(db.cpu(), be.grad * gscale)
    print(f"({rows}, {dim}): rel L2 dgamma {eg:.3e}, dbeta {eb:.3e}")
    assert eg <= 1e-5 and eb <= 1e-5
    # dbeta is the documented order bit for bit
    np.testing.assert_array_equal(db.cpu().numpy(), chunked_colsum_f32(dyo.numpy(), ops.COLSUM_CHUNK) * np.float32(gscale))
    for t, lr, with_state in ((1, 1e-4, False), (7, 1e-4, True), (7, 0.0, True)):
        sg = gen(t)
        (_, mg0, vg0), (_, mb0, vb0) = _state((dim,), with_state, sg), _state((dim,), with_state, sg)
        gam, bet, mg, vg, mb, vb = (t_.clone().to(DEV) for t_ in (gamma0, beta0, mg0, vg0, mb0, vb0))
        a = ops.adamw_step(lr, t)
        dg2, db2 = ops.layernorm_wgrad_adamw(x.to(DEV), dyo.to(DEV), LN_EPS, gam, bet, mg, vg, mb, vb, a, gscale=gscale, return_grad=True)
        assert torch.equal(dg2, dg) and torch.equal(db2, db)
        _check_update(gam, mg, vg, gamma0, mg0, vg0, dg.cpu().numpy(), a, lr)
        _check_update(bet, mb, vb, beta0, mb0, vb0, db.cpu().numpy(), a, lr)


# ---- 5. ViTTrainer.gradients against float64 autograd through the oracle ---------------------------------------------------------------
def make_trainer(embed, depth, img, seed=43, **kw):
    from nested_diffusion_amd.train_transformer import ViTTrainer
    vp = ref_cpu.init_vit_params(embed=embed, depth=depth, patch=16, img=img, seed=seed)
    return ViTTrainer(vp, num_classes=2, num_heads=embed // 64, **kw), vp


def oracle_gradients(vp, x, labels, heads, depth):
    p64 = {k: v.double().clone().requires_grad_() for k, v in vp.items()}
    logits = ref_cpu.vit_full_forward(p64, x.double(), heads, depth)
    F.cross_entropy(logits, labels).backward()
    return {k: v.grad for k, v in p64.items()}, logits.detach()


@pytest.mark.parametrize("embed,depth,img,B", [(128, 2, 32, 3), (128, 1, 16, 1), (768, 2, 224, 2)])
def test_gradients_follow_float64_autograd(embed, depth, img, B):
    trainer, vp = make_trainer(embed, depth, img)
    g = gen(B + img)
    x, labels = torch.rand(B, 3, img, img, generator=g), torch.randint(0, 2, (B,), generator=g)
    before = trainer.state_dict()
    grads, loss, logits = trainer.gradients(x, labels)
    assert torch.equal(logits, trainer.vit.forward(x.to(DEV)))                # bit for bit
    ref, logits64 = oracle_gradients(vp, x, labels, embed // 64, depth)
    assert sorted(grads) == sorted(vp)
    np.testing.assert_allclose(loss.cpu().double().numpy(), F.cross_entropy(logits64, labels, reduction="none").numpy(), rtol=1e-4, atol=1e-6)
    worst = {}
    for k in vp:
        assert tuple(grads[k].shape) == tuple(vp[k].shape), k
        worst[k] = rel_l2(grads[k].cpu(), ref[k])              # whole tensors only (the k-third of a qkv bias gradient is rounding noise)
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:3]
    print(f"embed {embed}, depth {depth}, img {img}, B {B}: largest rel L2 {top}")
    assert top[0][1] <= 1e-4, top
    after = trainer.state_dict()
    assert trainer.t == 0 and all(torch.equal(before[k], after[k]) for k in before)      # nothing was updated
    with pytest.raises(ValueError):
        trainer.gradients(x, labels + 2)


# ---- 6. / 7. the step is the listing; the images follow the masters ------------------------------------------------------------------
def test_step_is_the_listing_and_images_follow_the_masters():
    from nested_diffusion_amd import ops
    from nested_diffusion_amd.mapping import VisionTransformer
    trainer, vp = make_trainer(128, 2, 32)
    g = gen(6)
    x, labels = torch.rand(3, 3, 32, 32, generator=g), torch.tensor([1, 0, 1])
    images = [(t.data.data_ptr(), t) for t in [*trainer.vit.p.values(), *trainer.vit._wT.values(), trainer.vit.pe_w] if isinstance(t, ops.SplitMatrix)]
    assert len(images) == 2 * (4 * 2 + 1)                     # every block Linear and the patch embedding, and their transposes
    for step in (1, 2):
        w0 = trainer.state_dict()
        m0 = {k: t.cpu().clone() for k, t in trainer.m.items()}
        v0 = {k: t.cpu().clone() for k, t in trainer.v.items()}
        grads, loss, logits = trainer.gradients(x, labels)
        loss_sum, n_correct = trainer.step(x, labels)
        assert trainer.t == step
        assert float(loss_sum) == float(loss.sum()) and int(n_correct) == int((logits.argmax(1).cpu() == labels).sum())
        a = ops.adamw_step(1e-4, step, 0.1)
        w1 = trainer.state_dict()
        assert list(w1) == list(vp)
        for k in vp:
            we, me, ve = adamw_f32(w0[k].numpy(), m0[k].numpy(), v0[k].numpy(), grads[k].cpu().numpy(), a)
            np.testing.assert_array_equal(trainer.m[k].cpu().numpy(), me, err_msg=k)
            np.testing.assert_array_equal(trainer.v[k].cpu().numpy(), ve, err_msg=k)
            np.testing.assert_array_equal(w1[k].numpy(), we, err_msg=k)
            assert not np.array_equal(we, w0[k].numpy()), k   # every parameter moved
    # the images were rewritten in place, from the masters
    assert all(t.data.data_ptr() == p for p, t in images)
    sd = trainer.state_dict()
    assert sd["patch_embed.proj.weight"].dim() == 4
    fresh = VisionTransformer(sd, 2, DEV)
    xd = x.to(DEV)
    assert torch.equal(trainer.vit.forward(xd), fresh.forward(xd))
    lg_t, dx_t, loss_t = trainer.vit.input_grad(xd, labels)
    lg_f, dx_f, loss_f = fresh.input_grad(xd, labels)
    assert torch.equal(lg_t, lg_f) and torch.equal(dx_t, dx_f) and torch.equal(loss_t, loss_f)
    assert float(dx_t.abs().max()) > 0.0


def test_input_grad_is_still_the_chain_it_was():
    """VisionTransformer.input_grad on test_gpu_attack's 'tiny' model, against its listing restated here from the operators (the launches
    of _input_backward and _block_grad as they stood before the trainer kept the fp32 gradients): bit for bit."""
    from nested_diffusion_amd import ops
    from nested_diffusion_amd.mapping import VisionTransformer
    vp = ref_cpu.init_vit_params(embed=128, depth=5, patch=16, img=32, seed=3)
    vit = VisionTransformer(vp, 2, DEV)
    g = gen(12)
    x, labels = torch.rand(4, 3, 32, 32, generator=g).to(DEV), torch.randint(0, 2, (4,), generator=g)
    logits, dx, loss = vit.input_grad(x, labels)
    lg, cls_in, recs, B, N, H, W = vit._forward_recorded(x)
    wT, p = vit.transposed_weights(), vit.p
    dcls, loss2 = ops.xent_head_grad(lg, labels, p["head.weight"])
    dcls = ops.layernorm_grad(cls_in, p["norm.weight"], dcls, LN_EPS)
    dy = torch.zeros(B, N, 128, device=DEV)
    dy[:, 0] = dcls
    dy = dy.reshape(B * N, 128)
    dy_img = ops.split_rows(dy)
    for i in reversed(range(5)):
        r, pre = recs[i], f"blocks.{i}."
        dg = ops.gemm_split(dy_img, wT[pre + "mlp.fc2.weight"])
        dh = ops.gemm_split(ops.gelu_grad_split(r["u"], dg), wT[pre + "mlp.fc1.weight"])
        dx2, dx2_img = ops.layernorm_grad(r["x2"], p[pre + "norm2.weight"], dh, LN_EPS, residual=dy, want_split=True)
        da = ops.gemm_split(dx2_img, wT[pre + "attn.proj.weight"])
        dqkv = ops.attention_grad(r["qkv"], r["o"], da, B, N, 2, want_out=False, want_split=True)
        dh = ops.gemm_split(dqkv, wT[pre + "attn.qkv.weight"])
        dy, dy_img = ops.layernorm_grad(r["x"], p[pre + "norm1.weight"], dh, LN_EPS, residual=dx2, want_split=True)
    dpatch = dy.reshape(B, N, 128)[:, 1:].reshape(-1, 128).contiguous()
    want = ops.unpatchify(ops.gemm_split(dpatch, wT["patch_embed"]), B, 3, H, W, 16)
    assert torch.equal(lg, logits) and torch.equal(loss2, loss) and torch.equal(want, dx) and float(dx.abs().max()) > 0.0


def test_gradients_are_still_the_pass_they_were():
    """ViTTrainer.gradients against its listing restated here from the operators (the launches of the gradient-only pass as they stood
    while the trainer carried its own copy of the backward chain): bit for bit, every key, the loss and the logits.  B * N = 15 token
    rows: one short of every 16-, 32- and 64-row tile and chunk of the chain."""
    from nested_diffusion_amd import ops
    trainer, vp = make_trainer(128, 2, 32)
    g = gen(21)
    x, labels = torch.rand(3, 3, 32, 32, generator=g), torch.randint(0, 2, (3,), generator=g)
    grads, loss, logits = trainer.gradients(x, labels)
    vit, p, E, heads = trainer.vit, trainer.vit.p, 128, 2
    images, lab = x.to(DEV), labels.to(DEV)
    lg, cls_in, recs, B, N, H, W = vit._forward_recorded(images)
    assert (B, N) == (3, 5)
    wT, gscale, want = vit.transposed_weights(), 1.0 / B, {}

    def gemm(k, dy, inp):
        want[k] = ops.gemm_tn_adamw(dy, inp, None, None, None, None, gscale=gscale, return_grad=True).reshape(vp[k].shape)

    def colsum(k, dy):
        want[k] = ops.colsum_adamw(dy, None, None, None, None, gscale=gscale, return_grad=True).reshape(vp[k].shape)

    def norm(pre, inp, gr):
        want[pre + ".weight"], want[pre + ".bias"] = ops.layernorm_wgrad_adamw(inp, gr, LN_EPS, None, None, None, None, None, None, None,
                                                                               gscale=gscale, return_grad=True)

    _, loss2, dlogits = ops.ensemble_xent_grad(lg[None], lab)
    dlogits = dlogits[0]
    dcls, _ = ops.xent_head_grad(lg, lab, p["head.weight"])
    cls = ops.layernorm(cls_in, p["norm.weight"], p["norm.bias"], LN_EPS)
    dcls_in = ops.layernorm_grad(cls_in, p["norm.weight"], dcls, LN_EPS)
    gemm("head.weight", dlogits, cls)
    colsum("head.bias", dlogits)
    norm("norm", cls_in, dcls)
    dy = torch.zeros(B, N, E, device=DEV)
    dy[:, 0] = dcls_in
    dy = dy.reshape(B * N, E)
    dy_img = ops.split_rows(dy)
    for i in reversed(range(2)):
        r, pre = recs[i], f"blocks.{i}."
        dg = ops.gemm_split(dy_img, wT[pre + "mlp.fc2.weight"])
        du, du_img = ops.gelu_grad_split(r["u"], dg, want_out=True)
        dh2 = ops.gemm_split(du_img, wT[pre + "mlp.fc1.weight"])
        dx2, dx2_img = ops.layernorm_grad(r["x2"], p[pre + "norm2.weight"], dh2, LN_EPS, residual=dy, want_split=True)
        da = ops.gemm_split(dx2_img, wT[pre + "attn.proj.weight"])
        dqkv, dqkv_img = ops.attention_grad(r["qkv"], r["o"], da, B, N, heads, want_out=True, want_split=True)
        dh1 = ops.gemm_split(dqkv_img, wT[pre + "attn.qkv.weight"])
        dx, dx_img = ops.layernorm_grad(r["x"], p[pre + "norm1.weight"], dh1, LN_EPS, residual=dx2, want_split=True)
        gelu, _ = ops.gelu_split(r["u"], want_out=True)
        h2 = ops.layernorm(r["x2"], p[pre + "norm2.weight"], p[pre + "norm2.bias"], LN_EPS)
        h1 = ops.layernorm(r["x"], p[pre + "norm1.weight"], p[pre + "norm1.bias"], LN_EPS)
        gemm(pre + "mlp.fc2.weight", dy, gelu)
        colsum(pre + "mlp.fc2.bias", dy)
        gemm(pre + "mlp.fc1.weight", du, h2)
        colsum(pre + "mlp.fc1.bias", du)
        norm(pre + "norm2", r["x2"], dh2)
        gemm(pre + "attn.proj.weight", dx2, r["o"])
        colsum(pre + "attn.proj.bias", dx2)
        gemm(pre + "attn.qkv.weight", dqkv, h1)
        colsum(pre + "attn.qkv.bias", dqkv)
        norm(pre + "norm1", r["x"], dh1)
        dy, dy_img = dx, dx_img
    tokg = dy.reshape(B, N, E)
    colsum("pos_embed", dy.reshape(B, N * E))
    colsum("cls_token", tokg[:, 0].contiguous())
    dpatch = tokg[:, 1:].reshape(-1, E).contiguous()
    gemm("patch_embed.proj.weight", dpatch, ops.patchify(images, 16))
    colsum("patch_embed.proj.bias", dpatch)
    assert sorted(want) == sorted(grads) == sorted(vp)
    assert torch.equal(lg, logits) and torch.equal(loss2, loss)
    for k in vp:
        assert torch.equal(grads[k], want[k]), k
        assert float(grads[k].abs().max()) > 0.0, k


# ---- 8. it learns ---------------------------------------------------------------------------------------------------------------------
def test_it_learns_eight_images():
    trainer, _ = make_trainer(128, 2, 32, seed=43)
    x = torch.rand(8, 3, 32, 32, generator=gen(9))
    labels = torch.tensor([0, 1, 1, 0, 1, 0, 0, 1])
    losses = []
    for _ in range(40):
        loss_sum, _ = trainer.step(x, labels)
        losses.append(loss_sum)
    logits = trainer.logits(x).cpu()
    first, last = float(losses[0]) / 8, float(F.cross_entropy(logits, labels))
    print(f"mean loss: first {first:.4f}, step 40 {float(losses[-1]) / 8:.5f}, after 40 steps {last:.5f}")
    assert trainer.t == 40 and last < 0.1 * first
    assert bool((logits.argmax(1) == labels).all())


# ---- 9. fit and the CLI ---------------------------------------------------------------------------------------------------------------
def _png_tree(root):
    from PIL import Image
    rng = np.random.RandomState(5)
    for split, n in (("training", 3), ("validation", 2)):
        for c, (lo, hi) in (("a", (0, 90)), ("b", (160, 255))):
            os.makedirs(os.path.join(root, split, c))
            for i in range(n):
                Image.fromarray(rng.randint(lo, hi, (32, 32, 3)).astype(np.uint8), "RGB").save(os.path.join(root, split, c, f"{i}.png"))


def test_fit_and_cli_write_a_checkpoint_the_loaders_read(tmp_path, capsys, monkeypatch):
    from nested_diffusion_amd import train_transformer as tt
    from nested_diffusion_amd.mapping import VisionTransformer, load_pickled
    root, out = str(tmp_path / "data"), str(tmp_path / "out")
    _png_tree(root)
    init = tt.init_state_dict(num_classes=2, embed=128, depth=1, patch=16, img=224, seed=2)
    # fit, with the validation logits noted at every save
    trainer = tt.ViTTrainer(init, num_classes=2, num_heads=2)
    train_loader, valid_loader = tt.make_loaders(root, "ChestXRay", "grayscaled", 2, 7)
    noted, save = {}, torch.save

    def noting_save(obj, path):
        noted["logits"] = torch.cat([trainer.logits(xb) for xb, _ in valid_loader]).cpu()
        save(obj, path)

    monkeypatch.setattr(torch, "save", noting_save)
    res = trainer.fit(train_loader, valid_loader, 2, out, "ChestXRay")
    monkeypatch.setattr(torch, "save", save)
    path = os.path.join(out, "vit_base_patch16_224_ChestXRay.pth")
    assert res["path"] == path and os.path.exists(path) and res["saved_epochs"] and res["saved_epochs"][0] == 0
    assert trainer.t == 2 * 3 and trainer.epoch == 2
    lines = capsys.readouterr().out.splitlines()
    assert [l.split(":")[0] for l in lines] == ["Epoch 0 Train Loss", "Epoch 0 Test Loss", "Epoch 1 Train Loss", "Epoch 1 Test Loss",
                                                "Model vit on ChestXRay best train Acc"]
    sd = load_pickled(path)
    assert list(sd) == list(init) and all(sd[k].shape == init[k].shape for k in init) and sd["patch_embed.proj.weight"].dim() == 4
    vit = VisionTransformer(sd, 2, DEV)
    again = torch.cat([vit.forward(xb.to(DEV)) for xb, _ in valid_loader]).cpu()
    assert torch.equal(again, noted["logits"])
    # the command line: the same two epochs from the same start under the same seed end in the same file
    ckpt, out2 = str(tmp_path / "init.pth"), str(tmp_path / "out2")
    torch.save(init, ckpt)
    res2 = tt.main(["--dataset", "ChestXRay", "--root_dir", root, "--out", out2, "--init", ckpt, "--seed", "7", "--epochs", "2",
                    "--batch_size", "2"])
    assert res2["path"] == os.path.join(out2, "vit_base_patch16_224_ChestXRay.pth") and res2["saved_epochs"] == res["saved_epochs"]
    assert capsys.readouterr().out.splitlines()[0] == f"Training vit on {root} with seed 7:"
    sd2 = load_pickled(res2["path"])
    assert all(torch.equal(sd[k], sd2[k]) for k in sd)
