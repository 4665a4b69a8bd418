"""Training of the mapping MLPs on the GPU: nd_linear_wgrad_adam (the weight gradient formed on the matrix pipe and Adam applied to the
packed images in registers), nd_bias_grad_adam, nd_unpack_rows, and MappingTrainer end to end against torch on the CPU."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import ref_cpu
from test_train_mapping_host import adam_f32

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ragged_shape():
    """(N, K) from the kernel's own plan: the last workgroup over K holds fewer column blocks than the others, the workgroups over the row
    blocks hold two row blocks each and the last of them one."""
    from nested_diffusion_amd import ops
    K = 16 * (ops.linear_wgrad_plan(16, 16)["kb_per_wg"] + 3)
    for nrb in range(3, 8192, 2):
        N = 16 * nrb - 11
        p = ops.linear_wgrad_plan(N, K)
        if p["rb_per_wg"] == 2:
            assert nrb % 2 == 1 and p["grid_y"] == (nrb + 1) // 2 and (K // 16) % p["kb_per_wg"] != 0 and p["grid_x"] == 2
            return N, K
    raise AssertionError("no shape with two row blocks per workgroup below 8192 row blocks")


def padding_rows(img):
    """the image rows N .. 16 * ceil(N / 16) of a PackedWeight: lane l = 16 q + c of a block holds row c"""
    nrb, nkb = (img.N + 15) // 16, img.K // 16
    return img.data.view(nrb, nkb, 4, 16, 4)[-1, :, :, img.N - 16 * (nrb - 1):, :]


# ---- 1. the gradient ------------------------------------------------------------------------------------------------------------------------
GRAD_SHAPES = [(1, 1, 16), (3, 2, 16), (30, 17, 48), (128, 16, 32), (30, 128, 2048), "ragged",
               (33, 17, 48), (50, 33, 304), (64, 16, 32), (65, 17, 48)]        # the 16-step kernel (33 <= M <= 64) and both of its edges


@pytest.mark.parametrize("shape", GRAD_SHAPES, ids=str)
def test_gradient_is_within_the_rounding_bound(shape):
    """(M + 2) 2^-24 sum_m |dy x| |gscale| per element: one rounding per product, M - 1 sums, one scale"""
    from nested_diffusion_amd import ops
    M, N, K = (30, *ragged_shape()) if shape == "ragged" else shape
    g = gen(M * 1000 + N)
    dy, x, gscale = torch.randn(M, N, generator=g), torch.randn(M, K, generator=g), 1.0 / 3.0
    w = ops.PackedWeight(torch.zeros(N, K, device=DEV))
    before = w.data.clone()
    gi = ops.linear_wgrad_adam(dy.to(DEV), x.to(DEV), w, None, None, None, gscale=gscale, return_grad=True)
    got = gi.unpack().cpu().double()
    ref = dy.double().t() @ x.double() * float(np.float32(gscale))
    bound = (M + 2) * U * (dy.double().abs().t() @ x.double().abs()) * float(np.float32(gscale))
    excess = ((got - ref).abs() - bound).max()
    print(f"{(M, N, K)}: max |g - g64| = {float((got - ref).abs().max()):.3e}, max bound = {float(bound.max()):.3e}")
    assert float(excess) <= 0.0, (M, N, K, float(excess))
    assert (gi.N, gi.K) == (N, K) and torch.equal(w.data, before)          # the gradient-only call writes nothing else
    if N % 16:
        assert bool((padding_rows(gi) == 0).all())


# ---- 2. the update, bit for bit -------------------------------------------------------------------------------------------------------------
def _update_case(M, N, K, t, lr, with_state, seed):
    from nested_diffusion_amd import ops
    g = gen(seed)
    dy, x = torch.randn(M, N, generator=g), torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) * 0.1
    m0 = torch.randn(N, K, generator=g) * 0.05 if with_state else torch.zeros(N, K)
    v0 = torch.rand(N, K, generator=g) * 0.01 if with_state else torch.zeros(N, K)
    w, m, v = ops.PackedWeight(W.to(DEV)), ops.PackedWeight(m0.to(DEV)), ops.PackedWeight(v0.to(DEV))
    a = ops.adam_step(lr, t)
    gi = ops.linear_wgrad_adam(dy.to(DEV), x.to(DEV), w, m, v, a, gscale=1.0 / M, return_grad=True)
    return W, m0, v0, w, m, v, gi, a


@pytest.mark.parametrize("M,N,K", [(3, 2, 16), (30, 17, 48), (50, 33, 304), (128, 33, 304)])
@pytest.mark.parametrize("t,lr,with_state", [(1, 1e-3, False), (7, 1e-3, True), (7, 0.0, True)])
def test_update_equals_the_float32_listing_bit_for_bit(M, N, K, t, lr, with_state):
    W, m0, v0, w, m, v, gi, a = _update_case(M, N, K, t, lr, with_state, 100 * t + N)
    G = gi.unpack().cpu().numpy()
    we, me, ve = adam_f32(W.numpy(), m0.numpy(), v0.numpy(), G, a)
    np.testing.assert_array_equal(m.unpack().cpu().numpy(), me)
    np.testing.assert_array_equal(v.unpack().cpu().numpy(), ve)
    np.testing.assert_array_equal(w.unpack().cpu().numpy(), we)
    if lr == 0.0:
        assert np.array_equal(w.unpack().cpu().numpy().view(np.uint32), W.numpy().view(np.uint32))
    else:
        assert not np.array_equal(we, W.numpy())
    for img in (w, m, v, gi):
        assert bool((padding_rows(img) == 0).all())


def test_bias_update_bit_for_bit_and_in_row_order():
    from nested_diffusion_amd import ops
    M, N = 30, 37
    dy = torch.randn(M, N, generator=gen(3))
    # columns whose float32 sum depends on the order: a large term, small ones it swallows, and its cancellation
    dy[:, 0] = 1.0
    dy[0, 0], dy[18, 0] = 2.0 ** 25, -2.0 ** 25
    dy[:, 5] = torch.tensor([1e8, 1.0, -1e8, 1.0] * 7 + [3.0, 5.0])
    acc = np.zeros(N, np.float32)
    for r in range(M):
        acc = acc + dy[r].numpy()
    rev = np.zeros(N, np.float32)
    for r in reversed(range(M)):
        rev = rev + dy[r].numpy()
    assert acc[0] != rev[0] and acc[5] != rev[5] and acc[0] != np.float32(dy[:, 0].double().sum())
    gscale = np.float32(1.0 / M)
    G = acc * gscale
    for t, lr, with_state in ((1, 1e-3, False), (7, 1e-3, True), (7, 0.0, True)):
        g = gen(t)
        b0 = torch.randn(N, generator=g)
        m0 = torch.randn(N, generator=g) * 0.05 if with_state else torch.zeros(N)
        v0 = torch.rand(N, generator=g) * 0.01 if with_state else torch.zeros(N)
        b, m, v = b0.to(DEV), m0.to(DEV), v0.to(DEV)
        ptrs = (b.data_ptr(), m.data_ptr(), v.data_ptr())
        a = ops.adam_step(lr, t)
        got = ops.bias_grad_adam(dy.to(DEV), b, m, v, a, gscale=1.0 / M, return_grad=True)
        np.testing.assert_array_equal(got.cpu().numpy(), G)
        be, me, ve = adam_f32(b0.numpy(), m0.numpy(), v0.numpy(), G, a)
        np.testing.assert_array_equal(m.cpu().numpy(), me)
        np.testing.assert_array_equal(v.cpu().numpy(), ve)
        np.testing.assert_array_equal(b.cpu().numpy(), be)
        assert ptrs == (b.data_ptr(), m.data_ptr(), v.data_ptr())
        if lr == 0.0:
            assert np.array_equal(b.cpu().numpy().view(np.uint32), b0.numpy().view(np.uint32))
    only = ops.bias_grad_adam(dy.to(DEV), None, None, None, None, gscale=1.0 / M, return_grad=True)
    np.testing.assert_array_equal(only.cpu().numpy(), G)
    with pytest.raises(ValueError):
        ops.bias_grad_adam(dy.to(DEV), None, None, None, None)
    with pytest.raises(ValueError):
        ops.bias_grad_adam(dy.to(DEV), torch.zeros(N + 1, device=DEV), torch.zeros(N, device=DEV), torch.zeros(N, device=DEV), ops.adam_step(1e-3, 1))


# ---- 3. the same bits twice -----------------------------------------------------------------------------------------------------------------
def test_two_runs_from_the_same_state_give_the_same_images():
    N, K = ragged_shape()
    runs = [_update_case(30, N, K, 7, 1e-3, True, 9) for _ in range(2)]
    for i in (3, 4, 5, 6):
        assert torch.equal(runs[0][i].data, runs[1][i].data)


# ---- 4. NaN containment ---------------------------------------------------------------------------------------------------------------------
def test_a_nan_stays_in_its_weight_row_or_column():
    from nested_diffusion_amd import ops
    M, N, K = 30, 37, 80
    g = gen(21)
    dy, x, W = torch.randn(M, N, generator=g), torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)

    def run(dy_, x_):
        w = ops.PackedWeight(W.to(DEV))
        m, v = w.zeros_like(), w.zeros_like()
        gi = ops.linear_wgrad_adam(dy_.to(DEV), x_.to(DEV), w, m, v, ops.adam_step(1e-3, 1), gscale=1.0 / M, return_grad=True)
        return [t.unpack().cpu() for t in (w, m, v, gi)], (w, m, v, gi)
    clean, _ = run(dy, x)
    bad_dy = dy.clone()
    bad_dy[4, 19] = float("nan")
    got, imgs = run(bad_dy, x)
    for c, t in zip(clean, got):
        assert bool(t[19].isnan().all())
        keep = torch.arange(N) != 19
        assert torch.equal(t[keep], c[keep])
    for img in imgs:
        assert bool((padding_rows(img) == 0).all())
    bad_x = x.clone()
    bad_x[29, 66] = float("nan")
    got, imgs = run(dy, bad_x)
    for c, t in zip(clean, got):
        assert bool(t[:, 66].isnan().all())
        keep = torch.arange(K) != 66
        assert torch.equal(t[:, keep], c[:, keep])
    for img in imgs:                                        # a NaN column of x does not reach the image's padding rows
        assert bool((padding_rows(img) == 0).all())


def test_padding_rows_stay_zero_at_eps_zero():
    """eps = 0 makes m / denom = 0 / 0 wherever the gradient and v are both 0: the padding rows are not updated at all, so they stay 0 and the
    next input gradient (a contraction over the image's rows) stays finite"""
    from nested_diffusion_amd import ops
    M, N, K = 6, 37, 48
    g = gen(23)
    dy, x, W = torch.randn(M, N, generator=g).to(DEV), torch.randn(M, K, generator=g).to(DEV), torch.randn(N, K, generator=g)
    w = ops.PackedWeight(W.to(DEV))
    m, v = w.zeros_like(), w.zeros_like()
    a = ops.adam_step(1e-3, 1, eps=0.0)
    gi = ops.linear_wgrad_adam(dy, x, w, m, v, a, gscale=1.0 / M, return_grad=True)
    for img in (w, m, v, gi):
        assert bool((padding_rows(img) == 0).all())
    we, me, ve = adam_f32(W.numpy(), np.zeros((N, K), np.float32), np.zeros((N, K), np.float32), gi.unpack().cpu().numpy(), a)
    np.testing.assert_array_equal(w.unpack().cpu().numpy(), we)
    assert bool(w.unpack().isfinite().all()) and bool(ops.linear_grad_input(dy, w).isfinite().all())


# ---- 5. in place: the pointer stays, the forward sees the new weights --------------------------------------------------------------------
def test_update_is_in_place_and_the_forward_streams_it():
    from nested_diffusion_amd import ops
    M, N, K = 6, 37, 304
    g = gen(31)
    dy, x, W = torch.randn(M, N, generator=g).to(DEV), torch.randn(M, K, generator=g).to(DEV), torch.randn(N, K, generator=g).to(DEV)
    w = ops.PackedWeight(W)
    m, v = w.zeros_like(), w.zeros_like()
    assert m.data.data_ptr() != v.data.data_ptr() != w.data.data_ptr() and (m.N, m.K, m.dtype) == (N, K, w.dtype)
    assert bool((m.data == 0).all()) and m.data.shape == w.data.shape
    ptrs = [t.data.data_ptr() for t in (w, m, v)]
    assert ops.linear_wgrad_adam(dy, x, w, m, v, ops.adam_step(1e-2, 1), gscale=1.0 / M) is None
    assert ptrs == [t.data.data_ptr() for t in (w, m, v)]
    W2 = w.unpack()
    assert not torch.equal(W2, W)
    bias = torch.randn(N, generator=g).to(DEV)
    assert torch.equal(ops.linear(x, w, bias, act="relu"), ops.linear(x, ops.PackedWeight(W2), bias, act="relu"))


def test_wrapper_refusals():
    from nested_diffusion_amd import _lib, ops
    W = torch.randn(32, 64, generator=gen(4)).to(DEV)
    w = ops.PackedWeight(W)
    m, v = w.zeros_like(), w.zeros_like()
    dy, x, a = torch.randn(4, 32, device=DEV), torch.randn(4, 64, device=DEV), ops.adam_step(1e-3, 1)
    before = w.data.clone()
    with pytest.raises(_lib.NdError, match="fp32"):
        ops.linear_wgrad_adam(dy, x, ops.PackedWeight(W, "f16"), m, v, a)
    with pytest.raises(_lib.NdError, match="fp32"):
        ops.PackedWeight(W, "f16").unpack()
    with pytest.raises(TypeError):
        ops.linear_wgrad_adam(dy, x, W, m, v, a)
    with pytest.raises(TypeError):
        ops.linear_wgrad_adam(dy, x, w, m.data, v, a)
    with pytest.raises(ValueError, match="128"):
        ops.linear_wgrad_adam(torch.randn(129, 32, device=DEV), torch.randn(129, 64, device=DEV), w, m, v, a)
    for bad_dy, bad_x in ((torch.randn(4, 31, device=DEV), x), (dy, torch.randn(4, 48, device=DEV)), (dy, torch.randn(3, 64, device=DEV)),
                          (torch.randn(0, 32, device=DEV), x)):
        with pytest.raises(ValueError):
            ops.linear_wgrad_adam(bad_dy, bad_x, w, m, v, a)
    with pytest.raises(ValueError, match="distinct"):
        ops.linear_wgrad_adam(dy, x, w, m, m, a)
    with pytest.raises(ValueError):
        ops.linear_wgrad_adam(dy, x, w, m, ops.PackedWeight(torch.zeros(16, 64, device=DEV)), a)
    with pytest.raises(ValueError, match="nothing"):
        ops.linear_wgrad_adam(dy, x, w, None, None, None)
    with pytest.raises(_lib.NdError):
        ops.linear_wgrad_adam(dy.cpu(), x, w, m, v, a)
    torch.cuda.synchronize()
    assert torch.equal(w.data, before) and bool((m.data == 0).all())


# ---- 6. unpack is the inverse of pack -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(2, 16), (17, 48), (128, 2048)])
def test_unpack_inverts_pack(N, K):
    from nested_diffusion_amd import ops
    W = torch.randn(N, K, generator=gen(N)).to(DEV)
    W[0, 0], W[-1, -1] = -0.0, float("inf")
    out = ops.PackedWeight(W).unpack()
    assert out.shape == (N, K) and torch.equal(out.view(torch.int32), W.view(torch.int32))


# ---- 7. one member's linear1, sampled ---------------------------------------------------------------------------------------------------
def test_production_shape_sampled_blocks():
    """N = 4096, K = 150528, M = 30, one step on images filled in place (7.4 GB).  For the update dy and x are small integers and gscale a
    power of two, so the gradient is exact in fp32 and the sampled blocks must equal float64 gradient + float32 listing bit for bit; a second,
    gradient-only launch on random dy and x checks the same blocks against the float64 gradient within the rounding bound."""
    from nested_diffusion_amd import _lib, ops
    free = torch.cuda.mem_get_info()[0]
    if free < 16 * 2 ** 30:
        pytest.skip(f"needs 16 GB of free device memory, {free / 2 ** 30:.1f} GB are free")
    M, N, K = 30, 4096, 150528
    nrb, nkb = N // 16, K // 16
    plan = ops.linear_wgrad_plan(N, K)

    def image(fill):
        t = object.__new__(ops.PackedWeight)
        t.N, t.K, t.dtype = N, K, _lib.ND_DTYPE_F32
        t.data = torch.empty(nrb * nkb * 256, dtype=torch.float32, device=DEV)
        fill(t.data)
        return t
    dg = torch.Generator(device=DEV)
    dg.manual_seed(5)
    w = image(lambda d: d.normal_(0.0, 0.05, generator=dg))
    m = image(lambda d: d.normal_(0.0, 0.01, generator=dg))
    v = image(lambda d: d.uniform_(0.0, 1e-4, generator=dg))
    assert w.data.numel() * 4 > 2 ** 31
    dy = torch.randint(-4, 5, (M, N), generator=gen(1)).float()
    x = torch.randint(-4, 5, (M, K), generator=gen(2)).float()
    # the blocks: first and last, both sides of every workgroup boundary of the plan (over K at the row blocks beside the boundaries over
    # the rows, and the other way round at the first and last column block), and 64 drawn with a fixed seed
    kbounds = [j * plan["kb_per_wg"] for j in range(1, plan["grid_x"])]
    rbounds = [j * plan["rb_per_wg"] for j in range(1, plan["grid_y"])]
    rows = sorted({0, nrb - 1, *[r for b in rbounds[:4] + rbounds[-4:] for r in (b - 1, b)]})
    blocks = {(0, 0), (nrb - 1, nkb - 1)}
    blocks |= {(r, k) for r in rows[:4] for b in kbounds for k in (b - 1, b)}
    blocks |= {(r, k) for b in rbounds for r in (b - 1, b) for k in (0, nkb - 1)}
    rr, kk = torch.randint(0, nrb, (64,), generator=gen(3)), torch.randint(0, nkb, (64,), generator=gen(4))
    blocks |= set(zip(rr.tolist(), kk.tolist()))
    blocks = torch.tensor(sorted(blocks))
    idx = ((blocks[:, 0] * nkb + blocks[:, 1]) * 256)[:, None] + torch.arange(256)[None, :]

    def sample(img):
        """[nb, 16 n, 16 k] of the sampled blocks: float (n, k) of a block sits at ((n + 16 (k // 4)) * 4 + k % 4"""
        blk = img.data[idx.to(DEV)].cpu()
        return blk.view(-1, 4, 16, 4).permute(0, 2, 1, 3).reshape(-1, 16, 16).numpy()
    w0, m0, v0 = sample(w), sample(m), sample(v)
    ptr = w.data.data_ptr()
    a = ops.adam_step(1e-3, 7)
    ops.linear_wgrad_adam(dy.to(DEV), x.to(DEV), w, m, v, a, gscale=2.0 ** -5)
    dyb = torch.stack([dy[:, r * 16:(r + 1) * 16] for r in blocks[:, 0].tolist()]).double()
    xb = torch.stack([x[:, k * 16:(k + 1) * 16] for k in blocks[:, 1].tolist()]).double()
    G64 = torch.einsum("bmn,bmk->bnk", dyb, xb) * 2.0 ** -5
    G = G64.float()
    assert torch.equal(G.double(), G64)
    we, me, ve = adam_f32(w0, m0, v0, G.numpy(), a)
    np.testing.assert_array_equal(sample(m), me)
    np.testing.assert_array_equal(sample(v), ve)
    np.testing.assert_array_equal(sample(w), we)
    assert w.data.data_ptr() == ptr and len(blocks) >= 64 and not np.array_equal(we, w0)
    # the rounding of the accumulation at this shape: random dy and x, the gradient alone (m and v are done with and freed first), the same
    # blocks against the float64 gradient within the bound of test_gradient_is_within_the_rounding_bound
    del m, v
    dy, x = torch.randn(M, N, generator=gen(6)), torch.randn(M, K, generator=gen(7))
    gi = ops.linear_wgrad_adam(dy.to(DEV), x.to(DEV), w, None, None, None, gscale=1.0 / M, return_grad=True)
    dyb = torch.stack([dy[:, r * 16:(r + 1) * 16] for r in blocks[:, 0].tolist()]).double()
    xb = torch.stack([x[:, k * 16:(k + 1) * 16] for k in blocks[:, 1].tolist()]).double()
    gs = float(np.float32(1.0 / M))
    G64 = torch.einsum("bmn,bmk->bnk", dyb, xb) * gs
    bound = (M + 2) * U * torch.einsum("bmn,bmk->bnk", dyb.abs(), xb.abs()) * gs
    err = (torch.from_numpy(sample(gi)).double() - G64).abs()
    print(f"production shape, random data: max |g - g64| = {float(err.max()):.3e}, max bound = {float(bound.max()):.3e}")
    assert float((err - bound).max()) <= 0.0
    assert np.array_equal(sample(w), we)                                    # the gradient-only call left the weight alone


# ---- 8. end to end at tiny dims -----------------------------------------------------------------------------------------------------------
C, IMG, HIDDEN, LR = 3, 32, (32, 16, 16), 1e-2


@pytest.fixture(scope="module")
def tiny_vit():
    from nested_diffusion_amd.mapping import VisionTransformer
    vp = ref_cpu.init_vit_params(embed=128, depth=3, patch=16, img=IMG, num_classes=C, seed=3)
    return VisionTransformer(vp, 2, DEV), vp


def tiny_data(n=18, seed=11):
    """class-dependent images: a fixed pattern per class under uniform noise"""
    g = gen(seed)
    y = (torch.arange(n) % C)[torch.randperm(n, generator=g)]
    base = torch.rand(C, 3, IMG, IMG, generator=g)
    return 0.7 * base[y] + 0.3 * torch.rand(n, 3, IMG, IMG, generator=g), y


def make_trainer(vit, **kw):
    from nested_diffusion_amd.train_mapping import MappingTrainer
    return MappingTrainer(vit, 1, num_classes=C, lr=LR, seed=0, in_features=(IMG // 16) ** 2 * 128, hidden=HIDDEN, **kw)


def torch_run(sd, feats, labels, dtype, steps):
    layers = []
    for i in range(1, 5):
        W = sd[f"linear{i}.weight"]
        lin = torch.nn.Linear(W.shape[1], W.shape[0])
        lin.weight.data, lin.bias.data = W.clone(), sd[f"linear{i}.bias"].clone()
        layers += [lin] + ([torch.nn.ReLU()] if i < 4 else [])
    net = torch.nn.Sequential(*layers).to(dtype)
    opt = torch.optim.Adam(net.parameters(), lr=LR)
    losses = []
    for s in range(steps):
        b = s % len(feats)
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(net(feats[b].to(dtype)), labels[b])
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return np.array(losses, dtype=np.float64)


def test_trainer_follows_torch_adam_on_the_cpu(tiny_vit):
    """30 steps over three fixed batches of 6.  The GPU loss trajectory stays within 8 x (torch float32's largest deviation from torch
    float64) + 1e-6 of the float64 trajectory, both torch runs starting from the trainer's own initial weights and reading the GPU's own
    prefix features; the loss more than halves."""
    vit, _ = tiny_vit
    x, y = tiny_data()
    tr = make_trainer(vit)
    assert tr.model.in_features == 512 and [tr.model.p[f"linear{i}.weight"].N for i in range(1, 5)] == [32, 16, 16, 3]
    sd0 = tr.state_dict()
    for i, fan_in in zip(range(1, 5), (512, 32, 16, 16)):          # nn.Linear's default draw
        for s in ("weight", "bias"):
            t = sd0[f"linear{i}.{s}"]
            assert float(t.abs().max()) <= 1 / math.sqrt(fan_in) and float(t.abs().max()) > 0.5 / math.sqrt(fan_in)
    assert abs(float(sd0["linear1.weight"].mean())) < 0.01 / math.sqrt(512) * 10
    batches = [(x[i:i + 6], y[i:i + 6]) for i in (0, 6, 12)]
    feats = [tr.features(b.to(DEV)).cpu() for b, _ in batches]
    ptrs = [tr.model.p[f"linear{i}.weight"].data.data_ptr() for i in range(1, 5)]
    got, correct = [], []
    for s in range(30):
        loss_sum, n_ok = tr.step(*batches[s % 3])
        assert loss_sum.is_cuda and n_ok.is_cuda and loss_sum.dim() == 0 and n_ok.dim() == 0
        got.append(loss_sum)
        correct.append(n_ok)
    got = torch.stack(got).cpu().double().numpy() / 6
    assert tr.t == 30 and ptrs == [tr.model.p[f"linear{i}.weight"].data.data_ptr() for i in range(1, 5)]
    l64 = torch_run({k: v.double() for k, v in sd0.items()}, feats, [b[1] for b in batches], torch.float64, 30)
    l32 = torch_run(sd0, feats, [b[1] for b in batches], torch.float32, 30)
    yard = float(np.abs(l32 - l64).max())
    dev = float(np.abs(got - l64).max())
    print(f"GPU vs float64: {dev:.3e}; torch float32 vs float64: {yard:.3e}; loss {l64[0]:.4f} -> {l64[-1]:.4f} (GPU {got[0]:.4f} -> {got[-1]:.4f})")
    assert l64[-1] < 0.5 * l64[0] and got[-1] < 0.5 * got[0]
    assert dev <= 8 * yard + 1e-6, (dev, yard)
    assert all(0 <= int(c) <= 6 for c in correct)


def test_fit_writes_a_checkpoint_the_loaders_read(tiny_vit, tmp_path, capsys):
    from nested_diffusion_amd.mapping import Classifier, load_pickled
    vit, _ = tiny_vit
    x, y = tiny_data()
    xv, yv = tiny_data(12, seed=12)
    train = [(x[i:i + 6], y[i:i + 6]) for i in (0, 6, 12)]
    valid = [(xv[:7], yv[:7]), (xv[7:], yv[7:])]
    tr = make_trainer(vit, step_size=1, gamma=0.5)
    hist = tr.fit(train, valid, 2, str(tmp_path))
    out = capsys.readouterr().out
    assert out.count("Train Loss:") == 2 and out.count("Test Loss:") == 2 and "Epoch 1 Test Loss" in out and "best train Acc" in out
    path = os.path.join(str(tmp_path), "MLPs", "block_1.pth")
    assert hist["path"] == path and os.path.exists(path) and hist["saved_epochs"]
    assert tr.epoch == 2 and tr.t == 6 and tr.lr == LR / 4
    sd = load_pickled(path)
    assert sorted(sd) == sorted(Classifier.KEYS) and sd["linear1.weight"].shape == (32, 512) and sd["linear4.bias"].shape == (C,)
    # the file holds the weights of the last epoch that improved: a second trainer (same seed: the same bits) stopped after that epoch
    last = hist["saved_epochs"][-1]
    if last != 1:
        tr = make_trainer(vit, step_size=1, gamma=0.5)
        tr.fit(train, valid, last + 1, str(tmp_path / "again"))
        capsys.readouterr()
    clf = Classifier(sd, DEV)
    for xb, _ in valid:
        assert torch.equal(clf(tr.features(xb.to(DEV))), tr.logits(xb.to(DEV)))
    loss, acc = tr.evaluate(valid)
    assert math.isfinite(loss) and acc == hist["best_acc"]


def test_a_batch_of_129_is_refused_by_name(tiny_vit):
    vit, _ = tiny_vit
    tr = make_trainer(vit)
    before = tr.model.p["linear4.weight"].data.clone()
    with pytest.raises(ValueError, match="at most 128 rows"):
        tr.step(torch.zeros(129, 3, IMG, IMG), torch.zeros(129, dtype=torch.int64))
    assert tr.t == 0 and torch.equal(tr.model.p["linear4.weight"].data, before)
    with pytest.raises(ValueError, match="at least one"):
        tr.step(torch.zeros(0, 3, IMG, IMG), torch.zeros(0, dtype=torch.int64))
    with pytest.raises(ValueError, match="labels"):
        tr.step(torch.zeros(4, 3, IMG, IMG), torch.zeros(3, dtype=torch.int64))
    assert tr.t == 0 and torch.equal(tr.model.p["linear4.weight"].data, before)


def test_cli_trains_on_an_image_tree_and_load_conditioner_accepts_it(tmp_path, capsys):
    """python -m nested_diffusion_amd.train_mapping's main() for two epochs on a small image tree on disk (224 x 224 after the loader's
    resize, a two-block ViT of width 128): the checkpoint lands beside the ViT and load_conditioner builds a conditioner from both."""
    from PIL import Image
    from nested_diffusion_amd import train_mapping
    from nested_diffusion_amd.mapping import load_conditioner
    g = gen(8)
    for split, n in (("training", 5), ("validation", 3)):
        for ci, cls in enumerate(("NORMAL", "PNEUMONIA")):
            d = tmp_path / "data" / split / cls
            d.mkdir(parents=True)
            for i in range(n):
                a = (torch.rand(40, 40, 3, generator=g) * 100 + 100 * ci).to(torch.uint8).numpy()
                Image.fromarray(a, "RGB").save(str(d / f"{i}.png"))
    out = tmp_path / "models"
    out.mkdir()
    vp = ref_cpu.init_vit_params(embed=128, depth=2, patch=16, img=224, num_classes=2, seed=3)
    torch.save(vp, str(out / "vit_base_patch16_224_ChestXRay.pth"))
    hist = train_mapping.main(["--dataset", "ChestXRay", "--root_dir", str(tmp_path / "data"), "--mn_idx", "0", "--seed", "1", "--epochs", "2",
                               "--batch_size", "4", "--vit", str(out / "vit_base_patch16_224_ChestXRay.pth"), "--out", str(out)])
    text = capsys.readouterr().out
    assert "Training Mapping Network 0" in text and text.count("Train Loss:") == 2
    assert os.path.exists(str(out / "MLPs" / "block_0.pth")) and hist["saved_epochs"]
    cond = load_conditioner(str(out), "ChestXRay", DEV)
    assert len(cond.mlps) == 1 and cond.mlps[0].in_features == 196 * 128
    logits = cond.compute_guiding_prediction(torch.rand(2, 3, 224, 224, generator=g).to(DEV), include_full_vit=False)
    assert logits[0].shape == (2, 2) and bool(logits[0].isfinite().all())
