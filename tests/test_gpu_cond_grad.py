"""The gradient through the mapping networks on the GPU: nd_linear_bwd (the input gradient of a frag16-packed Linear, read in place),
nd_ensemble_xent_bwd (the ensemble's loss head), GuidingConditioner.input_grad against float64 autograd through the oracle, and the
gradient attacks pointed at a ConditionerTarget."""
import os

import pytest
import torch
import yaml

from oracle import ref_cpu
from test_gpu_attack import TAU, agree_except_near_zero, f64, oracle_step, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 8 / 255


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(shape, seed):
    return torch.randint(-4, 5, shape, generator=gen(seed)).float()


def make_gate(M, K, seed):
    """a post-ReLU activation: positives, and exact +0.0 / -0.0 entries (ReLU'(0) = 0 for both)"""
    g = torch.randn(M, K, generator=gen(seed)).clamp_min(0.0)
    g[::2, ::3] = 0.0
    g[1::2, 1::3] = -0.0
    g[0, 0] = 1.0
    return g


def raw_linear_bwd(dy, pw, gate, add, out, M=None, N=None, K=None, dtype=None):
    """nd_linear_bwd as the ABI takes it (no host checks): returns rc"""
    from nested_diffusion_amd import _lib
    p = lambda t: t if t is None or isinstance(t, int) else t.data_ptr()     # noqa: E731
    return _lib.load().nd_linear_bwd(p(dy), pw.data.data_ptr(), p(gate), p(add), p(out), dy.shape[0] if M is None else M,
                                     pw.N if N is None else N, pw.K if K is None else K, pw.dtype if dtype is None else dtype,
                                     torch.cuda.current_stream().cuda_stream)


# ---- 1. exact case ------------------------------------------------------------------------------------------------------------------
MS = (1, 15, 16, 17, 32, 33, 128)


@pytest.mark.parametrize("N,K,Ms", [(2, 16, MS), (3, 48, MS), (16, 16, MS), (17, 32, MS), (48, 592, MS), (32, 16496, MS), (128, 2048, MS),
                                    (2048, 4096, (32,))])
def test_linear_bwd_integers_are_exact(N, K, Ms):
    from nested_diffusion_amd import ops
    W = ints((N, K), 1000 + N + K)
    pw = ops.PackedWeight(W.to(DEV))
    for M in Ms:
        dy, add, gate = ints((M, N), 7 * M + N), ints((M, K), 11 * M + K), make_gate(M, K, M + K)
        prod = dy.double() @ W.double()                       # every partial sum is an integer of magnitude <= 16 N <= 2^16: exact in fp32
        masked = torch.where(gate > 0, prod, torch.zeros_like(prod))
        d, a, g = dy.to(DEV), add.to(DEV), gate.to(DEV)
        assert torch.equal(ops.linear_grad_input(d, pw).cpu().double(), prod), (M, "plain")
        assert torch.equal(ops.linear_grad_input(d, pw, gate=g).cpu().double(), masked), (M, "gate")
        assert torch.equal(ops.linear_grad_input(d, pw, add=a).cpu().double(), prod + add.double()), (M, "add")
        assert torch.equal(ops.linear_grad_input(d, pw, gate=g, add=a).cpu().double(), masked + add.double()), (M, "gate+add")
        out = a.clone()                                       # add is out
        assert raw_linear_bwd(d, pw, g, out, out) == 0
        assert torch.equal(out.cpu().double(), masked + add.double()), (M, "add is out")


# ---- 2. random fp32 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(17, 50, 48), (33, 300, 592), (128, 1000, 2048), (32, 2048, 4096)])
def test_linear_bwd_random_is_within_the_fma_chain_bound(M, N, K, record_property):
    """|err| <= (N + 3) 2^-24 ((|dy| . |W|) + |add|) per element: the forward-error bound of an N-term fmaf chain (gamma_N ~ N u, u = 2^-24,
    on sum |dy_n W_n|) plus one rounding each for the gate select (exact) and the add, and the final store."""
    from nested_diffusion_amd import ops
    g = gen(M + N + K)
    dy, W, add = torch.randn(M, N, generator=g), torch.randn(N, K, generator=g) / N ** 0.5, torch.randn(M, K, generator=g)
    gate = make_gate(M, K, 5)
    out = ops.linear_grad_input(dy.to(DEV), ops.PackedWeight(W.to(DEV)), gate=gate.to(DEV), add=add.to(DEV)).cpu().double()
    ref = torch.where(gate > 0, dy.double() @ W.double(), torch.zeros(M, K, dtype=torch.float64)) + add.double()
    bound = (N + 3) * 2.0 ** -24 * (dy.double().abs() @ W.double().abs() + add.double().abs())
    ratio = float(((out - ref).abs() / bound).max())
    record_property("worst_err_over_bound", ratio)
    print(f"M={M} N={N} K={K}: worst |err| / bound = {ratio:.3e}")
    assert ratio <= 1.0


# ---- 3. NaN and padding ---------------------------------------------------------------------------------------------------------------
def test_linear_bwd_nan_row_and_unread_padding():
    from nested_diffusion_amd import ops
    M, N, K, r = 33, 17, 32, 20
    W, dy = torch.randn(N, K, generator=gen(1)), torch.randn(M, N, generator=gen(2))
    pw = ops.PackedWeight(W.to(DEV))
    clean = ops.linear_grad_input(dy.to(DEV), pw)
    dy_nan = dy.clone()
    dy_nan[r, 5] = float("nan")
    out = ops.linear_grad_input(dy_nan.to(DEV), pw)
    assert bool(out[r].isnan().all())
    keep = [i for i in range(M) if i != r]
    assert torch.equal(out[keep], clean[keep]) and bool(out[keep].isfinite().all())
    # M = 17: rows 17 .. 31 of the second row tile and columns n = 17 .. 31 of every row are operands of the MFMA; neither is read
    M = 17
    buf = torch.full((M * N + 4096,), float("nan"), device=DEV)
    buf[:M * N] = dy[:M].to(DEV).reshape(-1)
    got = torch.empty(M, K, device=DEV)
    assert raw_linear_bwd(buf[:M * N].view(M, N), pw, None, None, got) == 0
    assert bool(got.isfinite().all()) and torch.equal(got, clean[:M])
    # the same with N % 4 == 0, the float4 dy loader: rows m >= M and quads n >= N take a clamped address and are zeroed, never used
    for N4 in (16, 32):
        W4, dy4 = torch.randn(N4, K, generator=gen(3)), torch.randn(33, N4, generator=gen(4))
        pw4 = ops.PackedWeight(W4.to(DEV))
        clean4 = ops.linear_grad_input(dy4.to(DEV), pw4)
        buf = torch.full((M * N4 + 4096,), float("nan"), device=DEV)
        buf[:M * N4] = dy4[:M].to(DEV).reshape(-1)
        got = torch.empty(M, K, device=DEV)
        assert buf.data_ptr() % 16 == 0 and raw_linear_bwd(buf[:M * N4].view(M, N4), pw4, None, None, got) == 0
        assert bool(got.isfinite().all()) and torch.equal(got, clean4[:M]), N4


# ---- 4. invariance --------------------------------------------------------------------------------------------------------------------
def test_linear_bwd_rows_do_not_depend_on_the_batch():
    from nested_diffusion_amd import ops
    N, K = 48, 592
    g = gen(9)
    W = torch.randn(N, K, generator=g)
    pw = ops.PackedWeight(W.to(DEV))
    dy, add, gate = torch.randn(130, N, generator=g).to(DEV), torch.randn(130, K, generator=g).to(DEV), make_gate(130, K, 3).to(DEV)
    full = ops.linear_grad_input(dy[:33], pw, gate=gate[:33], add=add[:33])
    for b in range(33):
        assert torch.equal(ops.linear_grad_input(dy[b:b + 1], pw, gate=gate[b:b + 1], add=add[b:b + 1])[0], full[b]), b
    assert torch.equal(ops.linear_grad_input(dy[:33], pw, gate=gate[:33], add=add[:33]), full)
    big = ops.linear_grad_input(dy, pw, gate=gate, add=add)           # M = 130: two launches inside ops
    two = torch.cat([ops.linear_grad_input(dy[s:e], pw, gate=gate[s:e], add=add[s:e]) for s, e in ((0, 128), (128, 130))])
    assert torch.equal(big, two) and torch.equal(big[:33], full)
    assert torch.equal(ops.linear_grad_input(dy, pw, gate=gate, add=add), big)


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------
def test_linear_bwd_refusals():
    from nested_diffusion_amd import _lib, ops
    W = torch.randn(32, 64, generator=gen(4)).to(DEV)
    pw = ops.PackedWeight(W)
    dy = torch.randn(4, 32, device=DEV)
    out = torch.full((129, 64), 7.0, device=DEV)
    with pytest.raises(_lib.NdError, match="fp32"):
        ops.linear_grad_input(dy, ops.PackedWeight(W, "f16"))
    assert raw_linear_bwd(dy, pw, None, None, out, dtype=_lib.ND_DTYPE_F16) != 0
    odd = object.__new__(ops.PackedWeight)                            # no image exists for K % 16 != 0: the wrapper refuses the shape
    odd.N, odd.K, odd.dtype, odd.data = 32, 24, _lib.ND_DTYPE_F32, pw.data
    with pytest.raises(ValueError, match="multiple of 16"):
        ops.linear_grad_input(dy, odd)
    assert raw_linear_bwd(dy, pw, None, None, out, K=24) != 0
    for kw in (dict(gate=torch.ones(4, 48, device=DEV)), dict(add=torch.ones(3, 64, device=DEV)), dict(gate=torch.ones(64, device=DEV))):
        with pytest.raises(ValueError):
            ops.linear_grad_input(dy, pw, **kw)
    for bad in (torch.randn(4, 31, device=DEV), torch.randn(32, device=DEV), torch.randn(0, 32, device=DEV)):
        with pytest.raises(ValueError):
            ops.linear_grad_input(bad, pw)
    with pytest.raises(_lib.NdError):
        ops.linear_grad_input(dy.cpu(), pw)
    with pytest.raises(TypeError):
        ops.linear_grad_input(dy, W)
    big = torch.randn(129, 32, device=DEV)
    assert raw_linear_bwd(big, pw, None, None, out) != 0              # M = 129 at the raw ABI
    assert raw_linear_bwd(big, pw, None, None, out, M=0) != 0
    odd_ptr = torch.ones(4 * 64 + 1, device=DEV).data_ptr() + 1      # a gate / add address that is no float's
    assert raw_linear_bwd(dy, pw, odd_ptr, None, out) != 0 and raw_linear_bwd(dy, pw, None, odd_ptr, out) != 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                   # refused before any launch


# ---- 6. one member's real shape ---------------------------------------------------------------------------------------------------------
def test_linear_bwd_at_one_members_real_shape():
    """150528 -> 4096: a 2.47 GB image, byte offsets past 2^31.  W[n, k] = ((7 n + 13 k + (n k mod 5)) mod 9) - 4, formed on the device."""
    from nested_diffusion_amd import ops
    M, N, K = 2, 4096, 150528
    n = torch.arange(N, dtype=torch.int32, device=DEV)[:, None]
    k = torch.arange(K, dtype=torch.int32, device=DEV)[None, :]
    W = (((7 * n + 13 * k + (n * k) % 5) % 9) - 4).float()
    pw = ops.PackedWeight(W)
    assert pw.data.numel() * 4 > 2 ** 31
    cols = torch.cat([torch.arange(64), torch.arange(K - 64, K), torch.randint(0, K, (4096,), generator=gen(6))])
    Wc = W[:, cols.to(DEV)].cpu().double()
    del W
    dy = ints((M, N), 8)
    out = ops.linear_grad_input(dy.to(DEV), pw)
    assert torch.equal(out[:, cols.to(DEV)].cpu().double(), dy.double() @ Wc)


# ---- 7. the ensemble head -----------------------------------------------------------------------------------------------------------------
def head64(logits, labels):
    """(P, loss, dlogits) of the closed form in float64"""
    K, B, C = logits.shape
    p = torch.softmax(logits.double(), dim=2)
    P = p.mean(dim=0)
    py = p[:, torch.arange(B), labels]
    onehot = torch.nn.functional.one_hot(labels, C).double()
    return P, -torch.log(P[torch.arange(B), labels]), (py / py.sum(0))[:, :, None] * (p - onehot)


@pytest.mark.parametrize("K", [1, 3, 5, 32])
def test_ensemble_xent_grad_against_float64(K):
    from nested_diffusion_amd import ops
    B = 6
    for C in (2, 3, 7, 1024):
        g = gen(10 * K + C)
        logits = torch.randn(K, B, C, generator=g) * 3
        labels = torch.randint(0, C, (B,), generator=g)
        P, loss, d = ops.ensemble_xent_grad(logits.to(DEV), labels.to(DEV))
        P64, loss64, d64 = head64(logits, labels)
        assert rel_l2(P, P64) <= 1e-5 and rel_l2(loss, loss64) <= 1e-5 and rel_l2(d, d64) <= 1e-5, (K, C)
        if K == 1:
            sm = torch.softmax(logits[0].double(), dim=1) - torch.nn.functional.one_hot(labels, C).double()
            assert rel_l2(d[0], sm) <= 1e-5
        P_only, none_loss, none_d = ops.ensemble_xent_grad(logits.to(DEV))
        assert none_loss is None and none_d is None and torch.equal(P_only, P)


def test_ensemble_xent_grad_conventions():
    from nested_diffusion_amd import _lib, ops
    K, B, C = 3, 4, 5
    logits = torch.randn(K, B, C, generator=gen(12))
    labels = torch.tensor([0, 1, 2, 3])
    clean = ops.ensemble_xent_grad(logits.to(DEV), labels.to(DEV))
    # underflow: every member's p[b, y] is 0 in fp32
    under = logits.clone()
    under[:, 1, 1] = -200.0
    P, loss, d = ops.ensemble_xent_grad(under.to(DEV), labels.to(DEV))
    assert float(loss[1]) == float("inf") and bool((d[:, 1] == 0).all()) and float(P[1, 1]) == 0.0
    for b in (0, 2, 3):
        assert torch.equal(loss[b], clean[1][b]) and torch.equal(d[:, b], clean[2][:, b]) and torch.equal(P[b], clean[0][b])
    # a NaN logit in one member's row: the whole row is NaN in P, loss and every member's dlogits; the other rows are untouched
    nan = logits.clone()
    nan[1, 2, 0] = float("nan")
    P, loss, d = ops.ensemble_xent_grad(nan.to(DEV), labels.to(DEV))
    assert bool(P[2].isnan().all()) and bool(loss[2].isnan()) and bool(d[:, 2].isnan().all())
    for b in (0, 1, 3):
        assert torch.equal(loss[b], clean[1][b]) and torch.equal(d[:, b], clean[2][:, b]) and torch.equal(P[b], clean[0][b])
    # a label outside [0, C): refused by the wrapper; with check_labels=False the kernel gives loss NaN, dlogits 0 and P as usual
    bad = torch.tensor([0, 1, C, -1])
    with pytest.raises(ValueError, match="labels"):
        ops.ensemble_xent_grad(logits.to(DEV), bad.to(DEV))
    P, loss, d = ops.ensemble_xent_grad(logits.to(DEV), bad.to(DEV), check_labels=False)
    assert bool(loss[2:].isnan().all()) and bool((d[:, 2:] == 0).all()) and torch.equal(P, clean[0])
    assert torch.equal(loss[:2], clean[1][:2]) and torch.equal(d[:, :2], clean[2][:, :2])
    for shape in ((33, 2, 4), (2, 3, 1), (2, 3, 1025)):
        with pytest.raises(ValueError):
            ops.ensemble_xent_grad(torch.zeros(shape, device=DEV))
    lib = _lib.load()
    z = torch.zeros(2, 3, 4, device=DEV)
    assert lib.nd_ensemble_xent_bwd(z.data_ptr(), None, z.data_ptr(), None, None, 33, 3, 4, None) != 0
    assert lib.nd_ensemble_xent_bwd(z.data_ptr(), torch.zeros(3, dtype=torch.int64, device=DEV).data_ptr(), z.data_ptr(), None, None, 2, 3, 4, None) != 0


# ---- 8. end to end at tiny dims -------------------------------------------------------------------------------------------------------------
def build_model(C, img, widths):
    from nested_diffusion_amd.mapping import Classifier, GuidingConditioner, VisionTransformer
    vp = ref_cpu.init_vit_params(embed=128, depth=3, patch=16, img=img, num_classes=C, seed=3)
    mlps = [ref_cpu.init_classifier_params((img // 16) ** 2 * 128, widths, C, seed=10 + i) for i in range(3)]
    cond = GuidingConditioner(VisionTransformer(vp, 2, DEV), [Classifier(m, DEV) for m in mlps])
    return cond, vp, mlps


@pytest.fixture(scope="module")
def model2():
    return build_model(2, 32, (48, 32, 16))


@pytest.fixture(scope="module")
def model3():
    return build_model(3, 64, (80, 48, 16))


def ref64(vp, mlps, x, labels, members):
    """(P, loss, dx) of the selected members in float64: autograd through the oracle's compute_guiding_prediction"""
    xx = x.double().clone().requires_grad_(True)
    outs = ref_cpu.compute_guiding_prediction(f64(vp), [f64(m) for m in mlps], xx, 2, 3, full_vit=False)
    P = torch.stack([torch.softmax(outs[m], dim=1) for m in members]).mean(dim=0)
    loss = -torch.log(P[torch.arange(x.shape[0]), labels])
    loss.sum().backward()
    return P.detach(), loss.detach(), xx.grad


@pytest.mark.parametrize("which", ["model2", "model3"])
def test_conditioner_input_grad_against_float64_autograd(which, request, record_property):
    cond, vp, mlps = request.getfixturevalue(which)
    img, C = (32, 2) if which == "model2" else (64, 3)
    B = 4
    x = torch.rand(B, 3, img, img, generator=gen(21))
    labels = torch.arange(B) % C
    P, dx, loss, logits = cond.input_grad(x.to(DEV), labels.to(DEV))
    want = torch.stack(cond.compute_guiding_prediction(x.to(DEV), include_full_vit=False))
    assert torch.equal(logits, want)                                   # the recorded forward is the C-level sequence, bit for bit
    assert torch.equal(torch.stack(cond.compute_guiding_prediction_py(x.to(DEV), include_full_vit=False)), want)
    P64, loss64, g64 = ref64(vp, mlps, x, labels, [0, 1, 2])
    r = rel_l2(dx, g64)
    record_property("dx_rel_l2", r)
    print(f"{which}: conditioner input gradient rel L2 {r:.3e}, P {rel_l2(P, P64):.3e}, loss {rel_l2(loss, loss64):.3e}")
    assert rel_l2(P, P64) <= 1e-5 and rel_l2(loss, loss64) <= 1e-5
    assert r <= 1e-5
    assert dx.shape == x.shape and bool(dx.isfinite().all())
    for members in ([0, 2], [1]):
        Pm, dxm, lossm, logm = cond.input_grad(x.to(DEV), labels.to(DEV), members=members)
        assert torch.equal(logm, want[members])
        P64, loss64, g64 = ref64(vp, mlps, x, labels, members)
        rm = rel_l2(dxm, g64)
        record_property(f"dx_rel_l2_members_{'_'.join(map(str, members))}", rm)
        assert rel_l2(Pm, P64) <= 1e-5 and rel_l2(lossm, loss64) <= 1e-5 and rm <= 1e-5, members
    with pytest.raises(ValueError):
        cond.input_grad(x.to(DEV), labels.to(DEV), members=[3])
    with pytest.raises(ValueError, match="labels"):
        cond.input_grad(x.to(DEV), labels.to(DEV) + C)


def test_conditioner_input_grad_refuses_fp16_mode():
    from nested_diffusion_amd import _lib
    from nested_diffusion_amd.mapping import Classifier, GuidingConditioner, VisionTransformer
    vp = ref_cpu.init_vit_params(embed=128, depth=1, patch=16, img=32, num_classes=2, seed=3)
    m = ref_cpu.init_classifier_params(4 * 128, (64, 32, 32), 2, seed=10)
    cond = GuidingConditioner(VisionTransformer(vp, 2, DEV, "f16"), [Classifier(m, DEV, "f16")])
    with pytest.raises(_lib.NdError, match="fp32"):
        cond.input_grad(torch.rand(2, 3, 32, 32, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV))


# ---- 9. attacks on the target ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def attacked(model2):
    from nested_diffusion_amd.mapping import ConditionerTarget
    cond, vp, mlps = model2
    target = ConditionerTarget(cond)
    x = torch.rand(6, 3, 32, 32, generator=gen(5))
    labels = target.forward(x.to(DEV)).argmax(dim=1)                   # the GPU's own clean predictions
    return target, x, labels


def test_target_forward_is_the_averaged_softmax(attacked, model2):
    from nested_diffusion_amd.mapping import ConditionerTarget
    target, x, labels = attacked
    cond, vp, mlps = model2
    P = target(x.to(DEV))
    P64, _, _ = ref64(vp, mlps, x, labels.cpu(), [0, 1, 2])
    assert rel_l2(P, P64) <= 1e-5
    Pg, dx, loss = target.input_grad(x.to(DEV), labels)
    assert torch.equal(Pg, P)                                          # the scores-only call and the gradient call form the same P
    sub = ConditionerTarget(cond, members=[2, 0])
    assert rel_l2(sub(x.to(DEV)), ref64(vp, mlps, x, labels.cpu(), [2, 0])[0]) <= 1e-5


def test_fgsm_on_the_target(attacked, model2):
    from nested_diffusion_amd.attack import Attack
    target, x, labels = attacked
    cond, vp, mlps = model2
    _, _, g64 = ref64(vp, mlps, x, labels.cpu(), [0, 1, 2])
    adv, success = Attack(EPS, "FGSM", target).generate_attack(x.to(DEV), labels)
    ok, frac = agree_except_near_zero(adv, oracle_step(x, x, g64, EPS, EPS), g64)
    assert ok and frac > 0.9
    assert float((adv.cpu() - x).abs().max()) <= EPS * (1 + 1e-6) and float(adv.min()) >= 0 and float(adv.max()) <= 1
    loss0, loss1 = target.input_grad(x.to(DEV), labels)[2], target.input_grad(adv, labels)[2]
    print("FGSM loss rise per row:", (loss1 - loss0).cpu().tolist(), "fooled:", success.cpu().tolist())
    assert bool((loss1 > loss0).all())                                 # every row
    assert bool(success.all())                                         # float64 on this model and seed: every row rises by >= 0.02 and is fooled
    assert torch.equal(success, target(adv).argmax(dim=1) != labels)


def _check_attack(make, x, labels, target, eps, l2):
    adv = make()
    d = adv.cpu() - x
    if l2:
        assert float(d.flatten(1).norm(dim=1).max()) <= eps * (1 + 1e-5)
    else:
        assert float(d.abs().max()) <= eps * (1 + 1e-6)
    assert float(adv.min()) >= 0 and float(adv.max()) <= 1
    fooled = (target(adv).argmax(dim=1) != labels).cpu()
    unchanged = (adv.cpu() == x).flatten(1).all(dim=1)
    print("fooled:", fooled.tolist(), "unchanged:", unchanged.tolist())
    assert torch.equal(unchanged, ~fooled)                             # exactly the rows it did not fool come back unchanged
    assert torch.equal(make(), adv)                                    # run to run
    return fooled


def test_pgd_on_the_target(attacked):
    from nested_diffusion_amd.attack import Attack
    target, x, labels = attacked
    _check_attack(lambda: Attack(EPS, "PGD", target, seed=3).generate_attack(x.to(DEV), labels)[0], x, labels, target, EPS, False)


def test_l2pgd_on_the_target(attacked):
    from nested_diffusion_amd.attack import L2Attack
    target, x, labels = attacked
    eps = 2.0
    _check_attack(lambda: L2Attack(eps, "L2PGD", target, seed=3).generate_attack(x.to(DEV), labels)[0], x, labels, target, eps, True)


def test_autoattack_on_the_target(attacked):
    from nested_diffusion_amd.autoattack import AutoAttack
    target, x, labels = attacked
    atk = AutoAttack(target, eps=0.1, seed=1, version="custom", attacks_to_run=["apgd-ce"])
    _check_attack(lambda: atk.run_standard_evaluation(x.to(DEV), labels, bs=6), x, labels, target, 0.1, False)


def test_cw_on_the_target_refuses(attacked):
    from nested_diffusion_amd.attack import CarliniWagner
    with pytest.raises(NotImplementedError, match="Carlini"):
        CarliniWagner(1.0, attacked[0])


# ---- the tools ------------------------------------------------------------------------------------------------------------------------------
def test_test_atk_takes_an_attack_on_the_conditioner(tmp_path, monkeypatch):
    import nested_diffusion_amd.runner as runner_mod
    from nested_diffusion_amd.attack import Attack, apply_attack
    from nested_diffusion_amd.mapping import ConditionerTarget
    from test_gpu_attack_e2e import FLAGS, _run_main
    from test_gpu_cli import _write_run
    tmp = str(tmp_path)
    ypath, *_ = _write_run(tmp, T=6, K=5, B=3, img=32)
    batches = [(torch.rand(3, 3, 32, 32, generator=gen(40 + n)), torch.tensor([0, 1, n])) for n in (0, 1)]
    reports = {}
    orig_atk = runner_mod.Diffusion.test_atk

    def spy(self, test_loader=None, attack=None):
        atk = Attack(EPS, "PGD", ConditionerTarget(self.cond_pred_model), seed=3)
        orig_atk(self, test_loader=batches, attack=atk)
        reports["attack"] = self.last_report
        adv = [(apply_attack(atk, x.to(self.device), t.to(self.device), "PGD", first_image=3 * n).cpu(), t) for n, (x, t) in enumerate(batches)]
        assert all(not torch.equal(a, x) for (a, _), (x, _) in zip(adv, batches))
        orig_atk(self, test_loader=adv)
        reports["apply"] = self.last_report
        return orig_atk(self, test_loader=batches)

    monkeypatch.setattr(runner_mod.Diffusion, "test_atk", spy)
    assert _run_main(FLAGS + ["--config", ypath, "--doc", "ct", "--exp", os.path.join(tmp, "r")]) == 0
    assert set(reports) == {"attack", "apply"}
    for k in reports["attack"]:
        ta, tb = torch.as_tensor(reports["attack"][k]), torch.as_tensor(reports["apply"][k])
        assert torch.allclose(ta, tb, rtol=0, atol=0, equal_nan=True), k


def test_write_attacked_set_takes_the_target(tmp_path):
    from nested_diffusion_amd import main as nd_main
    from nested_diffusion_amd import make_attacks, mapping
    from nested_diffusion_amd.attack import Attack
    from test_gpu_cli import _write_image_tree, _write_run
    tmp = str(tmp_path)
    ypath, *_ = _write_run(tmp, T=6, K=5, B=3, img=224)
    dataroot = os.path.join(tmp, "data")
    _write_image_tree(dataroot)
    config = nd_main.dict2namespace(yaml.safe_load(open(ypath)))
    cond = mapping.load_conditioner(config.diffusion.trained_aux_cls_ckpt_path, "ChestXRay", DEV, num_heads=2)
    target = mapping.ConditionerTarget(cond, members=[0, 1])
    out = os.path.join(tmp, "attacked")
    n_ok = make_attacks.write_attacked_set(config, Attack(EPS, "FGSM", target), "FGSM", out, batch_size=4, dataroot=dataroot)
    tree = os.path.join(out, "Test_attacks_FGSM")
    assert 0 <= n_ok <= 7 and sum(len(f) for _, _, f in os.walk(tree)) == 7
    assert sorted(os.listdir(tree)) == ["NORMAL", "PNEUMONIA"]


def test_make_attacks_main_with_the_conditioner_target(tmp_path, capsys):
    from nested_diffusion_amd import make_attacks
    from test_gpu_cli import _write_image_tree, _write_run
    tmp = str(tmp_path)
    ypath, *_ = _write_run(tmp, T=6, K=5, B=3, img=224)               # embed 128: load_conditioner's default head count is 128 // 64 = 2
    dataroot = os.path.join(tmp, "data")
    _write_image_tree(dataroot)
    out = os.path.join(tmp, "attacked")
    argv = ["--config", ypath, "--attack_name", "FGSM", "--eps", str(EPS), "--out", out, "--dataroot", dataroot, "--batch_size", "4"]
    assert make_attacks.main(argv + ["--target", "conditioner", "--members", "0,2"]) == 0
    assert "7 images written" in capsys.readouterr().out
    tree = os.path.join(out, "Test_attacks_FGSM")
    assert sum(len(f) for _, _, f in os.walk(tree)) == 7
    cond_png = {f: open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(tree) for f in fs}
    out2 = os.path.join(tmp, "attacked_vit")                          # the default target is the full ViT's head: other gradients, other images
    assert make_attacks.main(argv[:7] + [out2] + argv[8:]) == 0
    vit_png = {f: open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(os.path.join(out2, "Test_attacks_FGSM")) for f in fs}
    assert cond_png.keys() == vit_png.keys() and any(cond_png[f] != vit_png[f] for f in cond_png)
