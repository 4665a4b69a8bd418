"""Edge cases of the mapping-MLP gradient and training kernels (csrc/nd_mlp_grad.hip: nd_linear_bwd, nd_ensemble_xent_bwd;
csrc/nd_mlp_train.hip: nd_linear_wgrad_adam, nd_bias_grad_adam; csrc/nd_pack.hip: nd_unpack_rows) and of MappingTrainer's loss head:

- the ensemble head element by element against the float64 closed form, over both sides of its stride-64 and stride-256 loops and uneven
  member counts, under a bound counted from the kernel's operations; confident logits up to a margin of 110; one member underflowing
  alone; the K >= 2 underflow convention; +inf and all -inf rows;
- the trainer's loss and dlogits are torch's cross-entropy at any margin (K = 1 is a log-softmax), per sample and through one whole Adam
  step on a batch that holds a sample wrong by more than 104;
- the weight gradient + Adam on a plan with two row blocks per workgroup and a ragged last workgroup, bit for bit; x / dy rows past M are
  never read; the Adam listing at the edges of fp32 (zeros, signed zeros, denormals, overflow, infinities, FLT_MAX) bit for bit;
- nd_bias_grad_adam over one and several workgroups inside guard zones; nd_unpack_rows past its 8192-workgroup cap; nd_linear_bwd's scalar
  dy loader reached through a dy base that is not 16-byte aligned;
- the eight parameter gradients of one step against float64 autograd, element by element.

Every reference is float64 (or the numpy float32 listing where the claim is "bit for bit")."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_cond_grad import head64, make_gate, raw_linear_bwd
from test_gpu_train_mapping import C as TINY_C
from test_gpu_train_mapping import LR, _update_case, make_trainer, padding_rows, ragged_shape, tiny_data, tiny_vit  # noqa: F401  (tiny_vit: fixture)
from test_train_mapping_host import adam_f32

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24                   # fp32 unit roundoff: one correctly rounded operation errs by at most U relative
TINY = 2.0 ** -126               # the absolute slack of a result in (or flushed from) the denormal range
ULP_FN = 2.0                     # expf / logf of the device library: within 1 ulp = 2 U relative
SECOND_ORDER = 1.0 + 2.0 ** -10  # the first-order sums below stand for products (1 + e1)(1 + e2)...: every e is < 2^-10
MARGINS = [0, 5, 15, 20, 40, 80, 90, 103, 110]
NAN = float("nan")
INF = float("inf")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(shape, seed):
    return torch.randint(-4, 5, shape, generator=gen(seed)).float()


def stream():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. the ensemble head, element by element ------------------------------------------------------------------------------------------------
def head_bounds(logits, labels):
    """Per-element error bounds of nd_ensemble_xent_bwd against the float64 closed form, counted from the kernel's listing (u = 2^-24, every
    fp32 operation correctly rounded except expf / logf, which the device library keeps within 1 ulp = 2 u).  All magnitudes are float64
    values of the same element; first-order terms, times (1 + 2^-10) for the products of (1 + e) factors.

    a member's terms  e_c = expf(l_c - mx): the subtraction rounds (|l_c - mx| u absolute, the same relative in e_c), expf 2 u:
                      eps_e(c) = (|l_c - mx| + 2) u
    its sum           ceil(C / 64) terms per lane then 6 butterfly steps: a term passes through at most ceil(C / 64) - 1 + 6 additions, and
                      carries its own eps_e:  eps_s = (ceil(C / 64) + 5) u + sum_c e_c eps_e(c) / s
    p_c = e_c / s     eps_p(c) = eps_e(c) + eps_s + u,  |dp_c| <= p_c eps_p(c) + 2^-126
    P_c               K terms in member order (K - 1 additions), one division:  |dP_c| <= mean_k |dp_kc| + K u P_c + 2^-126
    S = sum_k p_ky    |dS| <= sum_k |dp_ky| + (K - 1) u S,  eps_S = |dS| / S
    loss, K >= 2      -logf(S / K): the division u, the logarithm's argument off by eps_S + u relative, its result by 2 u relative:
                      |dloss| <= -log1p(-(eps_S + u)) + 2 u |loss|   (no bound once eps_S + u >= 1 / 2: S is denormal there)
    loss, K == 1      logf(s) - (l_y - mx): |dloss| <= eps_s + 2 u |log s| + u |l_y - mx| + u |loss|
    w_k = p_ky / S    |dw_k| <= (|dp_ky| + w_k |dS|) / S + u w_k      (K == 1: w = 1, no operation)
    d_kc              w_k (p_kc - [c == y]): at the label p - 1 is exact for p >= 1 / 2 and rounds by u |p - 1| below, and inherits |dp|
                      whole -- the error there is relative to p, not to the cancelled 1 - p:
                      |dd_kc| <= w_k (|dp_kc| + [c == y] u |p_kc - 1|) + |p_kc - [c == y]| |dw_k| + u |d_kc| + 2^-126"""
    K, B, C = logits.shape
    l = logits.double()
    rows = torch.arange(B)
    mx = l.max(dim=2, keepdim=True).values
    delta = (l - mx).abs()
    e = torch.exp(l - mx)
    s = e.sum(dim=2, keepdim=True)
    p = e / s
    eps_e = (delta + ULP_FN) * U
    eps_s = (math.ceil(C / 64) + 5) * U + (e * eps_e).sum(dim=2, keepdim=True) / s
    dp = p * (eps_e + eps_s + U) + TINY
    P = p.mean(dim=0)
    dP = dp.sum(dim=0) / K + K * U * P + TINY
    py, dpy = p[:, rows, labels], dp[:, rows, labels]
    S = py.sum(dim=0)
    dS = dpy.sum(dim=0) + (K - 1) * U * S
    loss = -torch.log(S / K)
    onehot = F.one_hot(labels, C).double()
    if K == 1:
        dloss = eps_s[0, :, 0] + ULP_FN * U * torch.log(s[0, :, 0]).abs() + U * delta[0, rows, labels] + U * loss.abs()
        dw = torch.zeros(K, B, dtype=torch.float64)
    else:
        arg = dS / S + U
        dloss = torch.where(arg < 0.5, -torch.log1p(-arg.clamp(max=0.5)), torch.full_like(arg, INF)) + ULP_FN * U * loss.abs()
        dw = (dpy + (py / S) * dS) / S + U * (py / S)
    w = py / S
    d = w[:, :, None] * (p - onehot)
    dd = w[:, :, None] * (dp + onehot * U * (p - 1).abs()) + (p - onehot).abs() * dw[:, :, None] + U * d.abs() + TINY
    return {"P": dP * SECOND_ORDER, "loss": dloss * SECOND_ORDER, "d": dd * SECOND_ORDER, "S": S, "p": p, "w": w}


def worst(got, ref, bound):
    """max |got - ref| / bound over the elements (bound > 0 everywhere; an infinite bound counts 0)"""
    r = (got.double().cpu() - ref).abs() / bound
    r = torch.where(torch.isinf(bound), torch.zeros_like(r), r)
    return float(r.max())


@pytest.mark.parametrize("K", [1, 2, 4, 5, 31, 32])
@pytest.mark.parametrize("C", [2, 63, 64, 65, 255, 256, 257, 1000, 1024])
def test_ensemble_head_sweep_element_by_element(C, K, record_property):
    """C on both sides of the wave loop's stride (64) and of the column loop's (256), K filling the four waves unevenly and up to the last
    LDS slot, B = 1 and 70: P, loss and every member's dlogits within head_bounds of the float64 closed form, element by element."""
    from nested_diffusion_amd import ops
    ratios = {"P": 0.0, "loss": 0.0, "d": 0.0}
    for B in (1, 70):
        g = gen(100000 * K + 100 * C + B)
        logits = torch.randn(K, B, C, generator=g) * 3
        labels = torch.randint(0, C, (B,), generator=g)
        labels[0] = C - 1                                              # the last column is some row's label
        P, loss, d = ops.ensemble_xent_grad(logits.to(DEV), labels.to(DEV))
        P64, loss64, d64 = head64(logits, labels)
        bd = head_bounds(logits, labels)
        for name, got, ref in (("P", P, P64), ("loss", loss, loss64), ("d", d, d64)):
            r = worst(got, ref, bd[name])
            ratios[name] = max(ratios[name], r)
            assert r <= 1.0, (name, K, B, C, r)
        assert torch.equal(ops.ensemble_xent_grad(logits.to(DEV))[0], P)
    for name, r in ratios.items():
        record_property(f"worst_{name}_err_over_bound", r)
    print(f"K={K} C={C}: worst err / bound: P {ratios['P']:.3f}, loss {ratios['loss']:.3f}, dlogits {ratios['d']:.3f}")


def confident_rows(logits, labels, margin):
    """test_xent_head_grad_confident_logits' rows: the first half leads with the label by `margin`, the second half is confidently wrong
    (another class leads the label by `margin`)"""
    B, C = logits.shape
    rows = torch.arange(B)
    lead = logits.max(1).values + margin
    logits[rows[: B // 2], labels[: B // 2]] = lead[: B // 2]
    other = (labels[B // 2:] + 1) % C
    logits[rows[B // 2:], other] = logits[rows[B // 2:], labels[B // 2:]] + margin
    return logits


@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("C", [2, 10, 1000])
@pytest.mark.parametrize("K", [1, 3])
def test_ensemble_head_confident_logits(K, C, margin, record_property):
    """A trained head's margins, every member built like test_xent_head_grad_confident_logits' rows (the same labels for all members).
    K = 1 is the plain cross-entropy at every margin: loss and dlogits within head_bounds of float64, past the margin of 104 where
    expf(l_y - max) is 0 in fp32 (loss = the margin, dlogits = -1 at the label).
    K = 3: rows where every member surely underflows at the label (l_y - max <= -104.5: expf gives 0) follow the documented convention,
    loss +inf, dlogits 0, P as the scores-only call forms it; rows with S = sum_k p_ky >= 2^-116 (2^-126 is 2^-10 of it) are within head_bounds; between
    the two S is denormal, the bound is void, and either outcome is taken.  One more row: member 2 alone underflows (the label 120 behind),
    members 0 and 1 are wrong by 5: w_2 is exactly 0 (its dlogits row is all zero), the other two weights, read off the largest non-label
    column, sum to 1 within the bound, loss and dlogits finite."""
    from nested_diffusion_amd import ops
    B = 16
    g = gen(1000 * margin + 10 * C + K)
    labels = torch.randint(0, C, (B,), generator=g)
    logits = torch.stack([confident_rows(8 + 0.5 * torch.randn(B, C, generator=g), labels, margin) for _ in range(K)])
    if K == 3:                                                       # the row where one member underflows alone
        extra = 8 + 0.5 * torch.randn(K, 1, C, generator=g)
        y = int(torch.randint(0, C, (1,), generator=g))
        o = (y + 1) % C
        extra[:, 0, o] = extra.max(dim=2).values[:, 0] + 1.0
        extra[:2, 0, y] = extra[:2, 0, o] - 5.0
        extra[2, 0, y] = extra[2, 0, o] - 120.0
        logits, labels = torch.cat([logits, extra], dim=1), torch.cat([labels, torch.tensor([y])])
    Bt = logits.shape[1]
    rows = torch.arange(Bt)
    P, loss, d = (t.cpu() for t in ops.ensemble_xent_grad(logits.to(DEV), labels.to(DEV)))
    P64, loss64, d64 = head64(logits, labels)
    bd = head_bounds(logits, labels)
    assert worst(P, P64, bd["P"]) <= 1.0
    assert torch.equal(ops.ensemble_xent_grad(logits.to(DEV))[0].cpu(), P)
    trail = (logits[:, rows, labels] - logits.max(dim=2).values)     # fp32, as the kernel forms l_y - max
    sure_zero = (trail <= -104.5).all(dim=0) if K > 1 else torch.zeros(Bt, dtype=torch.bool)
    normal = bd["S"] >= 2.0 ** -116 if K > 1 else torch.ones(Bt, dtype=torch.bool)
    assert not bool((sure_zero & normal).any())
    r_loss = worst(loss[normal], loss64[normal], bd["loss"][normal])
    r_d = worst(d[:, normal], d64[:, normal], bd["d"][:, normal])
    record_property("worst_loss_err_over_bound", r_loss)
    record_property("worst_d_err_over_bound", r_d)
    record_property("rows_by_convention", int(sure_zero.sum()))
    print(f"K={K} C={C} margin={margin}: worst err / bound: loss {r_loss:.3f}, dlogits {r_d:.3f}; {int(sure_zero.sum())} rows underflow in every member")
    assert r_loss <= 1.0 and r_d <= 1.0
    assert bool(loss[normal].isfinite().all()) and bool(d[:, normal].isfinite().all())
    if K == 1:
        assert bool(normal.all())
        wrong = rows >= B // 2
        if margin >= 103:                                            # the margin is the loss, the label's gradient -1
            tol = 4 * U * logits[0].double().abs().max(1).values.clamp(min=1)
            assert bool(((loss.double() - margin).abs()[wrong] <= tol[wrong] + 2.0 ** -16).all())   # + the fp32 rounding of l_y + margin itself
            assert bool(((d[0, rows, labels].double() + 1).abs()[wrong] <= 4 * U).all())
        return
    # K >= 2: the documented convention where every member underflows
    assert bool((loss[sure_zero] == INF).all()) and bool((d[:, sure_zero] == 0).all())
    if margin >= 110:
        assert int(sure_zero.sum()) == B // 2
    between = ~(sure_zero | normal)                                  # S denormal: either the convention or a finite loss with bounded dlogits
    for b in rows[between].tolist():
        by_convention = float(loss[b]) == INF and bool((d[:, b] == 0).all())
        bounded = math.isfinite(float(loss[b])) and float(loss[b]) > 80 and worst(d[:, b], d64[:, b], bd["d"][:, b]) <= 1.0
        assert by_convention or bounded, (b, float(loss[b]))
    # the row where member 2 underflows alone
    b = Bt - 1
    assert bool(normal[b]) and bool((d[2, b] == 0).all()) and math.isfinite(float(loss[b]))
    c = int((bd["p"][0, b] * (1 - F.one_hot(labels[b], C))).argmax())                       # the leading non-label column (the same in every member)
    w_est = d[:2, b, c].double() / bd["p"][:2, b, c]
    w_tol = (bd["d"][:2, b, c] / bd["p"][:2, b, c]).sum()
    assert abs(float(w_est.sum()) - 1.0) <= float(w_tol), (w_est, w_tol)


@pytest.mark.parametrize("K", [1, 3])
def test_ensemble_head_infinite_rows_are_nan_and_stay_in_their_row(K):
    """A row whose largest logit is +inf (inf - inf) and a row that is all -inf (-inf - -inf) in one member are NaN in P, loss and every
    member's dlogits, as the header says of a NaN logit; the rows beside them keep their bits."""
    from nested_diffusion_amd import ops
    B, C = 5, 7
    logits = torch.randn(K, B, C, generator=gen(40 + K)) * 3
    labels = torch.tensor([0, 1, 2, 3, 6])
    clean = ops.ensemble_xent_grad(logits.to(DEV), labels.to(DEV))
    bad = logits.clone()
    bad[0, 1, 4] = INF
    bad[K - 1, 3, :] = -INF
    P, loss, d = ops.ensemble_xent_grad(bad.to(DEV), labels.to(DEV))
    for b in (1, 3):
        assert bool(P[b].isnan().all()) and bool(loss[b].isnan()) and bool(d[:, b].isnan().all()), b
    for b in (0, 2, 4):
        assert torch.equal(bits(P[b]), bits(clean[0][b])) and torch.equal(bits(loss[b]), bits(clean[1][b]))
        assert torch.equal(bits(d[:, b]), bits(clean[2][:, b]))
    assert torch.equal(bits(ops.ensemble_xent_grad(bad.to(DEV))[0][[0, 2, 4]]), bits(clean[0][[0, 2, 4]]))


# ---- 2. the trainer's loss is torch's cross-entropy --------------------------------------------------------------------------------------------
def torch_step(sd, feats, labels, dtype, lr=LR):
    """One step of torch.optim.Adam on the Classifier built from the state dict `sd`, mean cross-entropy on (feats, labels), in `dtype` on
    the CPU.  Returns (updated state dict, gradients by key, [dL/d(pre-activation of layer i)], [input of layer i], logits)."""
    ps = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    h = feats.to(dtype)
    xs, zs = [], []
    for i in range(1, 5):
        xs.append(h.detach())
        z = F.linear(h, ps[f"linear{i}.weight"], ps[f"linear{i}.bias"])
        z.retain_grad()
        zs.append(z)
        h = torch.relu(z) if i < 4 else z
    opt = torch.optim.Adam(list(ps.values()), lr=lr)
    F.cross_entropy(h, labels).backward()
    grads = {k: v.grad.clone() for k, v in ps.items()}
    opt.step()
    return {k: v.detach() for k, v in ps.items()}, grads, [z.grad for z in zs], xs, h.detach()


def test_trainer_loss_head_is_torch_cross_entropy_at_confident_logits(tiny_vit, monkeypatch, record_property):
    """The per-sample loss and dlogits MappingTrainer.step feeds to its backward pass (and the loss .evaluate reports), at the margins of
    test_xent_head_grad_confident_logits on both sides, against float64 F.cross_entropy(reduction='none') and softmax - onehot under that
    test's bounds: 4 * 2^-24 * max(1, max |logit|) for the loss; per element of d, 2 (ceil(C / 64) + 8) 2^-24 (p + onehot) + 2^-126 against
    torch's float32 softmax - onehot as there, and the same plus |l_c - max| 2^-24 p_c against float64 (fp32 rounds l_c - max before the
    exponential, in torch as in the kernel: at a margin of 40 that alone is 40 units of 2^-24 in p_c, more than the cited bound allows).
    linear4's weight image is zeroed and its bias set to the logits row, so the step's logits are that row exactly; batches of one make
    loss_sum the per-sample loss; dlogits is read where step hands it to nd_bias_grad_adam for linear4; the rate is 0 so the state stays.
    Confidently wrong by 103 and 110 the loss is the margin and the gradient at the label -1."""
    from nested_diffusion_amd import ops
    C = TINY_C
    vit, _ = tiny_vit
    tr = make_trainer(vit)
    tr.base_lr = 0.0
    tr.model.p["linear4.weight"].data.zero_()
    x, _ = tiny_data()
    img = x[:1].to(DEV)
    seen = []
    real = ops.bias_grad_adam

    def spy(dy, *a, **kw):
        seen.append(dy.detach().clone())
        return real(dy, *a, **kw)
    monkeypatch.setattr(ops, "bias_grad_adam", spy)
    g = gen(77)
    worst_loss = worst_d = 0.0
    for margin in MARGINS:
        for wrong in (False, True):
            z = 8 + 0.5 * torch.randn(C, generator=g)
            y = int(torch.randint(0, C, (1,), generator=g))
            if wrong:
                z[(y + 1) % C] = z[y] + margin
            else:
                z[y] = z.max() + margin
            tr.model.p["linear4.bias"].copy_(z.to(DEV))
            label = torch.tensor([y])
            del seen[:]
            loss_sum, n_ok = tr.step(img, label)
            assert len(seen) == 4 and tuple(seen[3].shape) == (1, C)
            assert torch.equal(tr.logits(img).cpu(), z[None])                  # the logits are the row itself
            d = seen[3][0].cpu().double()
            z64 = z.double()
            loss64 = float(F.cross_entropy(z64[None], label, reduction="none"))
            onehot = F.one_hot(label, C)[0].double()
            p64 = torch.softmax(z64, 0)
            d64 = p64 - onehot
            tol_loss = 4 * U * max(1.0, float(z64.abs().max()))
            p32 = torch.softmax(z, 0).double()
            tol_d = 2 * (math.ceil(C / 64) + 8) * U * (p32 + onehot) + TINY
            tol_d64 = tol_d + (z64 - z64.max()).abs() * U * p64                # + the rounding of l_c - max, which every fp32 softmax shares
            e_loss = abs(float(loss_sum) - loss64)
            e_eval = abs(tr.evaluate([(img, label)])[0] - loss64)
            e_d = max(float(((d - (p32 - onehot)).abs() / tol_d).max()), float(((d - d64).abs() / tol_d64).max()))
            worst_loss, worst_d = max(worst_loss, e_loss / tol_loss, e_eval / tol_loss), max(worst_d, e_d)
            print(f"margin {margin} {'wrong' if wrong else 'right'}: loss {float(loss_sum):.6f} (float64 {loss64:.6f}, bound {tol_loss:.2e}), "
                  f"d[label] {float(d[y]):.6g} (float64 {float(d64[y]):.6g}), worst |d - d64| / bound {e_d:.3f}")
            assert e_loss <= tol_loss and e_eval <= tol_loss, (margin, wrong, float(loss_sum), loss64)
            assert e_d <= 1.0, (margin, wrong, d, d64)
            if margin > 0:                                                     # (at margin 0 the label ties with the leader)
                assert int(n_ok) == (0 if wrong else 1)
            if wrong and margin >= 103:
                assert abs(float(loss_sum) - margin) <= tol_loss + 2.0 ** -16 and abs(float(d[y]) + 1.0) <= float(tol_d[y])
    record_property("worst_loss_err_over_bound", worst_loss)
    record_property("worst_d_err_over_bound", worst_d)


def test_one_step_with_a_sample_wrong_by_more_than_104_follows_torch_adam(tiny_vit, record_property):
    """linear4's bias set to (110, 0, 100), labels (0, 1, 2, 0, 1, 2): the samples labelled 1 trail the leading logit by about 110, where
    fp32 softmax gives the label probability 0; those labelled 0 and 2 are right / wrong by about 10.  One step; all eight updated tensors
    against one step of torch.optim.Adam in float64 from the same state on the GPU's own features, each within 8 x (torch float32's
    largest deviation from float64) + 1e-6 x the tensor's largest magnitude (the rule of test_trainer_follows_torch_adam_on_the_cpu).
    A head that drops the confidently wrong samples (no gradient where p_y underflows) moves the weights elsewhere or not at all."""
    vit, _ = tiny_vit
    tr = make_trainer(vit)
    tr.model.p["linear4.bias"].copy_(torch.tensor([110.0, 0.0, 100.0], device=DEV))
    x, _ = tiny_data()
    images, labels = x[:6], torch.tensor([0, 1, 2, 0, 1, 2])
    sd0 = tr.state_dict()
    feats = tr.features(images.to(DEV)).cpu()
    new64, _, _, _, logits64 = torch_step({k: v.double() for k, v in sd0.items()}, feats, labels, torch.float64)
    new32, _, _, _, _ = torch_step(sd0, feats, labels, torch.float32)
    trail = logits64.max(1).values - logits64[torch.arange(6), labels]
    assert int((trail > 104).sum()) == 2 and int(((trail > 1) & (trail < 20)).sum()) == 2 and int((trail == 0).sum()) == 2, trail
    loss_sum, _ = tr.step(images, labels)
    got = tr.state_dict()
    want_loss = float(F.cross_entropy(logits64, labels, reduction="sum"))
    print(f"loss_sum {float(loss_sum):.6f} (float64 {want_loss:.6f})")
    record_property("loss_sum", float(loss_sum))
    failed = []
    for k in sorted(sd0):
        dev = float((got[k].double() - new64[k]).abs().max())
        yard = float((new32[k].double() - new64[k]).abs().max())
        moved = float((new64[k] - sd0[k].double()).abs().max())
        record_property(f"{k}_gpu_vs_float64", dev)
        record_property(f"{k}_torch32_vs_float64", yard)
        print(f"{k}: GPU vs float64 {dev:.3e}; torch float32 vs float64 {yard:.3e}; the step moved it by {moved:.3e}")
        assert moved > 0.5 * LR
        if not dev <= 8 * yard + 1e-6 * float(new64[k].abs().max()):
            failed.append((k, dev, yard))
    assert math.isfinite(float(loss_sum)) and abs(float(loss_sum) - want_loss) <= 1e-5 * want_loss      # (a sanity check, not a rounding bound)
    assert not failed, failed


# ---- 3. weight gradient + Adam -----------------------------------------------------------------------------------------------------------------
def test_update_on_the_ragged_plan_bit_for_bit():
    """Two row blocks per workgroup, the last workgroup over the rows holding one, the last workgroup over K short, N % 16 != 0: w, m, v
    equal the float32 listing of the returned gradient bit for bit at t = 7 with state, the padding rows stay exactly 0.  The plan is
    asserted so that a change of its constants cannot silently stop covering the branch."""
    from nested_diffusion_amd import ops
    N, K = ragged_shape()
    plan = ops.linear_wgrad_plan(N, K)
    nrb, nkb = (N + 15) // 16, K // 16
    assert plan["rb_per_wg"] == 2 and nrb % 2 == 1 and plan["grid_y"] == (nrb + 1) // 2
    assert plan["grid_x"] >= 2 and 0 < nkb - (plan["grid_x"] - 1) * plan["kb_per_wg"] < plan["kb_per_wg"] and N % 16
    W, m0, v0, w, m, v, gi, a = _update_case(30, N, K, 7, 1e-3, True, 4242)
    G = gi.unpack().cpu().numpy()
    assert np.isfinite(G).all() and np.count_nonzero(G) > 0.99 * G.size
    we, me, ve = adam_f32(W.numpy(), m0.numpy(), v0.numpy(), G, a)
    for name, img, want in (("m", m, me), ("v", v, ve), ("w", w, we)):
        got = img.unpack().cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    assert not np.array_equal(we, W.numpy())
    for img in (w, m, v, gi):
        assert bool((padding_rows(img) == 0).all())


def raw_wgrad(dy, x, w, m, v, g, M, N, K, gscale, a):
    """nd_linear_wgrad_adam as the ABI takes it (no host copy of dy or x): returns rc"""
    from nested_diffusion_amd import _lib
    p = lambda t: None if t is None else (t.data.data_ptr() if hasattr(t, "N") else t.data_ptr())     # noqa: E731
    return _lib.load().nd_linear_wgrad_adam(p(dy), p(x), p(w), p(m), p(v), p(g), M, N, K, _lib.ND_DTYPE_F32, float(gscale),
                                            ctypes.byref(a) if a is not None else None, stream())


@pytest.mark.parametrize("M", [1, 3, 30, 33])
def test_wgrad_never_reads_rows_past_m(M):
    """x and dy are views of buffers that are NaN in front of and behind the M rows (4096 floats each side): the steps of four rows, whose
    last one reaches past M (M = 1, 3, 30 in the 8-step kernel, 33 in the 16-step one), zero-fill those operands in registers.  The
    gradient-only launch and the update give the bits of the launch on clean, exactly sized tensors, all finite."""
    from nested_diffusion_amd import ops
    N, K, G = 37, 304, 4096
    g = gen(500 + M)
    dy, x = torch.randn(M, N, generator=g), torch.randn(M, K, generator=g)
    W, m0, v0 = torch.randn(N, K, generator=g) * 0.1, torch.randn(N, K, generator=g) * 0.05, torch.rand(N, K, generator=g) * 0.01
    a = ops.adam_step(1e-3, 7)

    def guarded(t):
        buf = torch.full((t.numel() + 2 * G,), NAN, device=DEV)
        buf[G:G + t.numel()] = t.to(DEV).reshape(-1)
        return buf, buf[G:G + t.numel()].view(t.shape)

    def run(dy_, x_, update):
        w, m, v = (ops.PackedWeight(t.to(DEV)) for t in (W, m0, v0))
        gi = w.zeros_like()
        assert raw_wgrad(dy_, x_, w if update else None, m if update else None, v if update else None, gi, M, N, K, 1.0 / M,
                         a if update else None) == 0
        return [t.data.clone() for t in ((w, m, v, gi) if update else (gi,))]
    dbuf, dview = guarded(dy)
    xbuf, xview = guarded(x)
    assert dview.data_ptr() == dbuf.data_ptr() + 4 * G and xview.is_contiguous()
    for update in (False, True):
        clean = run(dy.to(DEV), x.to(DEV), update)
        got = run(dview, xview, update)
        for c, t in zip(clean, got):
            assert bool(t.isfinite().all()) and torch.equal(bits(t), bits(c)), (M, update)
        assert bool(got[-1].count_nonzero() > 0)
    assert bool(dbuf[:G].isnan().all()) and bool(dbuf[-G:].isnan().all()) and bool(xbuf[:G].isnan().all()) and bool(xbuf[-G:].isnan().all())


G_VALUES = [0.0, -0.0, 1e-20, -1e-20, 1e-22, 1e-40, -1e-40, 3e19, -3e19, INF, -INF, 1.0, -3.5e-3, 1e-30, 2.0 ** -63, 1e10]
W0_VALUES = [0.1, -0.0, 3.4028234663852886e38, -3.4028234663852886e38]
M0_VALUES = [0.0, -0.0, 0.05, -1e-40]
V0_VALUES = [0.0, -0.0, 1e-40, 1e-4]


def test_adam_listing_at_the_edges_of_fp32():
    """One launch, N = 16, K = 64, M = 4, gscale = 1 / 2.  dy[m, n] = [m == n % 4] selects a row of x, so the gradient of element (n, k) is
    x[n % 4, k] / 2: column k carries G_VALUES[k % 16] (its x entries are twice that; the two infinite columns hold the infinity in row 0
    only, so rows n % 4 == 0 get +-inf and the others 0 * inf = NaN), and element (n, k) starts from w0 = W0_VALUES[k // 16],
    m0 = M0_VALUES[n % 4], v0 = V0_VALUES[n // 4]: all 16 x 64 combinations (x = -0.0 gives g = +0.0: the contraction starts from +0).
    Together: g = 0 on v = 0 at the default eps; g * g denormal
    (1e-20, 1e-22) and zero (1e-30); g itself denormal, formed from a denormal MFMA operand; g * g = inf; g = +-inf and NaN; w0 = +-FLT_MAX;
    -0.0 in each of w0, m0, v0; v0 and m0 denormal.  w, m, v as uint32 equal the numpy float32 listing (which keeps denormals: asserted),
    NaN exactly where it is NaN."""
    from nested_diffusion_amd import ops
    N, K, M = 16, 64, 4
    f32 = np.float32
    gvals = np.array(G_VALUES, dtype=f32)
    x = np.zeros((M, K), dtype=f32)
    for k in range(K):
        gv = gvals[k % 16]
        if np.isinf(gv):
            x[0, k] = gv
        else:
            with np.errstate(over="raise"):
                x[:, k] = gv * f32(2.0)
    dy = np.zeros((M, N), dtype=f32)
    dy[np.arange(N) % 4, np.arange(N)] = 1.0
    n_idx, k_idx = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    W0 = np.array(W0_VALUES, dtype=f32)[k_idx // 16]
    m0 = np.array(M0_VALUES, dtype=f32)[n_idx % 4]
    v0 = np.array(V0_VALUES, dtype=f32)[n_idx // 4]
    with np.errstate(all="ignore"):
        G = x[n_idx % 4, k_idx] * f32(0.5) + f32(0.0)                     # the selected row, scaled; the accumulator starts from +0: -0 arrives as +0
        G[(n_idx % 4 != 0) & np.isinf(gvals[k_idx % 16])] = np.nan        # 0 * inf in the contraction
        a = ops.adam_step(1e-3, 7)
        we, me, ve = adam_f32(W0, m0, v0, G, a)
    # the reference keeps denormals, or the denormal cases would be void: v of g = 1e-20 on v0 = 0 is a non-zero denormal, and so is g = 1e-40
    probe = ve[0, 2]
    assert G[0, 2] == f32(1e-20) and v0[0, 2] == 0 and 0 < probe < f32(2.0 ** -126), probe
    assert 0 < G[0, 5] < f32(2.0 ** -126) and 0 < me[0, 5] < f32(2.0 ** -126)
    assert np.isinf(ve[0, 7]) and np.isinf(G[0, 9]) and np.isnan(G[1, 9]) and np.isnan(we[0, 9])
    w, m, v = (ops.PackedWeight(torch.from_numpy(t.copy()).to(DEV)) for t in (W0, m0, v0))
    gi = ops.linear_wgrad_adam(torch.from_numpy(dy).to(DEV), torch.from_numpy(x).to(DEV), w, m, v, a, gscale=0.5, return_grad=True)
    bad = []
    for name, img, want in (("g", gi, G), ("m", m, me), ("v", v, ve), ("w", w, we)):
        got = img.unpack().cpu().numpy()
        nan_g, nan_w = np.isnan(got), np.isnan(want)
        diff = (nan_g != nan_w) | (~nan_w & ~nan_g & (got.view(np.uint32) != want.view(np.uint32)))
        for n, k in zip(*np.nonzero(diff)):
            bad.append((name, int(n), int(k), float(G[n, k]), float(W0[n, k]), float(m0[n, k]), float(v0[n, k]), float(got[n, k]), float(want[n, k])))
    assert not bad, (len(bad), bad[:12])


# ---- 4. bias, unpack, the scalar dy loader -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 128])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 4096])
def test_bias_grad_adam_bit_for_bit_inside_guard_zones(N, M):
    """One workgroup short of full, exactly full, one element into a second (whose other 255 threads leave at n >= N), 16 workgroups; the
    column sum in the order m = 0 .. M - 1 and the float32 listing, with state, bit for bit.  b, m, v and g_out are views into one
    NaN-filled buffer, 61 floats of guard on each side of each (so none is 16-byte aligned): every guard keeps its bits."""
    from nested_diffusion_amd import _lib, ops
    g = gen(10 * N + M)
    dy = torch.randn(M, N, generator=g)
    b0, m0, v0 = torch.randn(N, generator=g), torch.randn(N, generator=g) * 0.05, torch.rand(N, generator=g) * 0.01
    acc = np.zeros(N, np.float32)
    for r in range(M):
        acc = acc + dy[r].numpy()
    gscale = np.float32(1.0 / 3.0)
    G = acc * gscale
    a = ops.adam_step(1e-3, 7)
    be, me, ve = adam_f32(b0.numpy(), m0.numpy(), v0.numpy(), G, a)
    GUARD = 61
    buf = torch.full((4 * N + 5 * GUARD,), NAN, device=DEV)
    buf.view(torch.int32)[:] = 0x7FC00000 + torch.arange(buf.numel(), dtype=torch.int32, device=DEV) % 4096      # NaNs told apart by their payload
    views = [buf[GUARD + i * (N + GUARD): GUARD + i * (N + GUARD) + N] for i in range(4)]
    for t, src in zip(views[:3], (b0, m0, v0)):
        t.copy_(src.to(DEV))
    mask = torch.ones(buf.numel(), dtype=torch.bool, device=DEV)
    for i in range(4):
        mask[GUARD + i * (N + GUARD): GUARD + i * (N + GUARD) + N] = False
    before = bits(buf)[mask].clone()
    d = dy.to(DEV)
    rc = _lib.load().nd_bias_grad_adam(d.data_ptr(), *(t.data_ptr() for t in views), M, N, float(gscale), ctypes.byref(a), stream())
    assert rc == 0
    for name, t, want in (("g", views[3], G), ("m", views[1], me), ("v", views[2], ve), ("b", views[0], be)):
        got = t.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, N, M)
    assert torch.equal(bits(buf)[mask], before) and int(mask.sum()) == 5 * GUARD


def test_unpack_rows_takes_a_second_trip_of_its_grid_stride_loop():
    """N = 523, K = 16384: 33 row blocks (the last holds 11 rows), a 34.6 MB image, more 16-byte pieces than 8192 workgroups x 256 threads
    move in one trip.  The output is the source bit for bit, with -0.0, inf and NaN payloads at the first elements, the last elements, and
    on both sides of the single-trip boundary (piece 8192 * 256 is lane 0 of block (32, 0): row 512, column 0; the piece in front of it
    is the last lane of block (31, 1023): row 511, columns 16380 .. 16383)."""
    from nested_diffusion_amd import _lib, ops
    N, K = 523, 16384
    assert _lib.load().nd_packed_bytes(N, K, _lib.ND_DTYPE_F32) // 16 > 8192 * 256
    dg = torch.Generator(device=DEV)
    dg.manual_seed(17)
    W = torch.randn(N, K, device=DEV, generator=dg)
    Wi = W.view(torch.int32)
    NEG_NAN = 0xFFC54321 - (1 << 32)
    payload = torch.tensor([-0x80000000, 0x7F800000, 0x7FC12345, NEG_NAN], dtype=torch.int32, device=DEV)   # -0.0, +inf, a NaN with a payload, a negative one
    for r, c in ((0, 0), (N - 1, K - 4), (512, 0), (511, K - 4), (522, 0), (16, 16)):
        Wi[r, c:c + 4] = payload
    pw = ops.PackedWeight(W)
    assert pw.data.numel() * 4 // 16 > 8192 * 256 and pw.data.numel() == 33 * 16 * K
    out = pw.unpack()
    assert out.shape == (N, K) and torch.equal(out.view(torch.int32), Wi)
    assert int(out.view(torch.int32)[512, 2]) == 0x7FC12345 and int(out.view(torch.int32)[N - 1, K - 1]) == NEG_NAN


@pytest.mark.parametrize("K", [16, 48])
@pytest.mark.parametrize("N", [16, 20, 32])
def test_linear_bwd_scalar_loader_on_a_misaligned_dy(N, K):
    """N % 4 == 0 with a dy base that is 4-byte but not 16-byte aligned (a row slice of a larger tensor): the launch takes the scalar dy
    loader.  dy starts 1, 2 and 3 floats into a 16-byte aligned buffer whose head and 4096-float tail are NaN; small-integer operands make
    the product exact: the result equals the aligned launch bit for bit and the float64 product, with and without a gate."""
    from nested_diffusion_amd import ops
    W = ints((N, K), 3000 + N + K)
    pw = ops.PackedWeight(W.to(DEV))
    for M in (1, 17, 33):
        dy, gate = ints((M, N), 13 * M + N), make_gate(M, K, M + N)
        prod = dy.double() @ W.double()
        masked = torch.where(gate > 0, prod, torch.zeros_like(prod))
        aligned = ops.linear_grad_input(dy.to(DEV), pw)
        aligned_gated = ops.linear_grad_input(dy.to(DEV), pw, gate=gate.to(DEV))
        assert torch.equal(aligned.cpu().double(), prod) and torch.equal(aligned_gated.cpu().double(), masked)
        for off in (1, 2, 3):
            buf = torch.full((off + M * N + 4096,), NAN, device=DEV)
            assert buf.data_ptr() % 16 == 0
            view = buf[off:off + M * N].view(M, N)
            view.copy_(dy.to(DEV))
            assert view.data_ptr() % 16 != 0 and view.data_ptr() % 4 == 0 and view.is_contiguous()
            for gt, want, want64 in ((None, aligned, prod), (gate.to(DEV), aligned_gated, masked)):
                got = torch.full((M, K), NAN, device=DEV)
                assert raw_linear_bwd(view, pw, gt, None, got) == 0
                assert bool(got.isfinite().all()) and torch.equal(bits(got), bits(want)), (M, off, gt is not None)
                assert torch.equal(got.cpu().double(), want64)
            assert bool(buf[:off].isnan().all()) and bool(buf[off + M * N:].isnan().all())


# ---- 5. one step, every parameter ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 6])
def test_one_step_gives_every_parameter_its_float64_gradient(B, tiny_vit, record_property):
    """in_features 512, hidden (32, 16, 16), C = 3: one step from the seeded initial state on ordinary logits.  After step 1 Adam's first
    moment is m = fl(g * fl(1 - beta1)) from m = 0, so each of the eight gradients is read back as m / fl(1 - beta1) and compared, element
    by element, with float64 autograd of the torch model built from the state dict taken before the step, on the GPU's own features.

    The bound of layer i, dy = dL/d(its pre-activation) [B, N] (the 1 / B of the mean inside), x = its input [B, K]:
        (B + 2) 2^-24 (|dy|^T |x|)[n, k]                                   the kernel's own rounding (B products, B - 1 sums, the scale)
      + 8 (ddy_i sum_m |x[m, k]| + dx_i sum_m |dy[m, n]|)                 what the fp32 rounding of dy and x themselves is worth
      + 2 * 2^-24 |g[n, k]| + 2^-149 / fl(1 - beta1)                      reading g back out of m
    ddy_i and dx_i are not taken from the GPU: they are the largest elementwise deviation of a torch float32 run of the same step on the
    CPU from the float64 run, over the whole dy_i (x_i) tensor, times the 8 of the suite's torch-float32 yardstick.  A per-element form of
    that term (|dy32 - dy64|^T |x|) would be one sample of a rounding error per element and is zero wherever torch happened to round
    exactly, so the tensor-wide maximum is used; the whole bound stays below 1e-3 of the tensor's largest gradient (asserted), orders of
    magnitude under a gate taken from the wrong layer or a bias left out.  The bias gradient is the same with x = 1."""
    vit, _ = tiny_vit
    tr = make_trainer(vit)
    x, y = tiny_data()
    images, labels = x[:B], y[:B]
    sd0 = tr.state_dict()
    feats = tr.features(images.to(DEV)).cpu()
    _, g64, dy64, x64, logits64 = torch_step({k: v.double() for k, v in sd0.items()}, feats, labels, torch.float64)
    _, _, dy32, x32, _ = torch_step(sd0, feats, labels, torch.float32)
    assert float(logits64.abs().max()) < 2.0
    loss_sum, _ = tr.step(images, labels)
    assert math.isfinite(float(loss_sum))
    omb1 = float(np.float32(1.0 - 0.9))
    for i in range(1, 5):
        dy, xx = dy64[i - 1], x64[i - 1]
        ddy = 8 * float((dy32[i - 1].double() - dy).abs().max())
        dx = 8 * float((x32[i - 1].double() - xx).abs().max())
        for kind in ("weight", "bias"):
            key = f"linear{i}.{kind}"
            if kind == "weight":
                got = tr.m[key].unpack().cpu().double() / omb1
                scale = dy.abs().t() @ xx.abs()
                sens = ddy * xx.abs().sum(0)[None, :] + dx * dy.abs().sum(0)[:, None]
            else:
                got = tr.m[key].cpu().double() / omb1
                scale = dy.abs().sum(0)
                sens = torch.full_like(scale, ddy * B)
            ref = g64[key]
            bound = (B + 2) * U * scale + sens + 2 * U * ref.abs() + 2.0 ** -149 / omb1
            ratio = float(((got - ref).abs() / bound).max())
            share = float(((B + 2) * U * scale + 2 * U * ref.abs()).sum() / bound.sum())
            record_property(f"{key}_worst_err_over_bound", ratio)
            print(f"B={B} {key}: worst |g - g64| / bound = {ratio:.3f} (max |g64| {float(ref.abs().max()):.3e}, max bound {float(bound.max()):.3e}, "
                  f"the kernel's own rounding is {share:.2f} of the bound)")
            assert got.shape == ref.shape and ratio <= 1.0, (key, ratio)
            assert float(bound.max()) <= 1e-3 * float(ref.abs().max())                      # the bound means something
