"""Training of the noise estimators on the GPU: nd_bn_train_fwd / nd_bn_train_bwd against float64 autograd, nd_sumsq against its documented
order, nd_clip_adam bit for bit against the listing, NoiseEstimatorTrainer against the float64 oracle and against the reference's own five
recorded steps (tests/golden/diffusion_train.npz), and Diffusion.train end to end on synthetic data.

The yardstick of every comparison with float64 is e32: the error of the same computation by torch in fp32 on the CPU.  The GPU may be
off by 4 e32 + 2^-24 max|ref| per tensor: another summation order over at most 128 terms, and one rounding of the result.  No test
hands a kernel an out-of-range timestep: the Python refusal is covered on the host (tests/test_diffusion_train_oracle_host.py).

Measured on an MI355X (each test prints its figures under -s): the BatchNorm kernels and the trainer's gradients use at most 0.84 of
their bound (an encoder weight gradient at the smallest dimensions); nd_sumsq is within 8.2e-8 relative of float64 (bound 2.1e-6);
nd_clip_adam and step() are bit-equal to the listing; over the five recorded steps the loss is within 4.8e-7 of the reference's, the
norm within 3.6e-5, the eval-mode output within 4.7e-5 and every compared parameter within 2.2 times the reference's own fp32 error
(the float64 oracle's deviation from the same recorded values: 6.0e-7, 1.7e-5, 4.0e-5), against the factor 8 allowed."""
import argparse
import glob
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _diffusion_train_oracle as oracle_mod
from oracle import ref_cpu
from test_train_mapping_host import adam_f32

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24


def gen(seed):
    return torch.Generator().manual_seed(seed)


def within(got, ref64, ref32, what, extra=0.0):
    """|got - ref64| <= 4 e32 + 2^-24 max|ref64| (+ extra); returns (error, bound) for the record"""
    ref64 = ref64.double()
    err = float((got.detach().cpu().double() - ref64).abs().max())
    e32 = float((ref32.double() - ref64).abs().max())
    bound = 4 * e32 + U * float(ref64.abs().max()) + extra
    print(f"    {what}: err {err:.3g}, e32 {e32:.3g}, bound {bound:.3g}")
    assert err <= bound, (what, err, bound)
    return err, bound


# ---- 1. BatchNorm in training mode, forward and backward -----------------------------------------------------------------------------------
def bn_reference(c, dtype):
    """torch autograd in `dtype` on the CPU: every output of the two entry points"""
    to = lambda a: None if a is None else a.to(dtype).clone().requires_grad_(True)    # noqa: E731
    u, gamma, beta, table, mul = to(c["u"]), to(c["gamma"]), to(c["beta"]), to(c.get("table")), to(c.get("mul"))
    rm, rv = c["rm"].to(dtype).clone(), c["rv"].to(dtype).clone()
    v = table[c["t"]] * u if table is not None else u
    mean, var = v.mean(0), v.var(0, unbiased=False)
    rstd = 1 / torch.sqrt(var + 1e-5)
    z = F.batch_norm(v, rm, rv, gamma, beta, True, 0.1, 1e-5)
    a = F.softplus(z) if c["act"] else z
    out = a * mul if mul is not None else a
    out.backward(c["dout"].to(dtype))
    r = {"out": out, "xhat": (v - mean) * rstd, "rstd": rstd, "rm": rm, "rv": rv, "du": u.grad, "dgamma": gamma.grad, "dbeta": beta.grad}
    if table is not None:
        r["dtable"] = table.grad
    if mul is not None:
        r["dmul"] = mul.grad
    return {k: t.detach() for k, t in r.items()}


def bn_case(M, N, gain, mul, act, T=10, t=None, seed=0, beta_shift=None):
    g = gen(seed + 1000 * M + N)
    c = {"u": torch.randn(M, N, generator=g) * 1.5 + 0.3, "gamma": torch.rand(N, generator=g) + 0.5, "beta": torch.randn(N, generator=g) * 0.5,
         "dout": torch.randn(M, N, generator=g), "rm": torch.randn(N, generator=g), "rv": torch.rand(N, generator=g) + 0.5, "act": act, "T": T}
    if beta_shift is not None:
        c["beta"][::2] += beta_shift                 # z = xhat * gamma + beta above the softplus threshold 20 in every other column
    if gain:
        c["table"] = torch.rand(T + 1, N, generator=g)
        if t is None:                                # 0 and T - 1 are both present; the other rows are drawn
            t = torch.randint(0, T, (M,), generator=g)
            t[0], t[-1] = 0, T - 1
        c["t"] = t.to(torch.int64)
    if mul:
        c["mul"] = torch.randn(M, N, generator=g)
    return c


BN_SHAPES = [(2, 1), (2, 16), (6, 48), (30, 272), (128, 64), (33, 4096)]
BN_CASES = {}
for _M, _N in BN_SHAPES:
    BN_CASES[f"{_M}x{_N}-plain"] = dict(M=_M, N=_N, gain=False, mul=False, act=False)
    BN_CASES[f"{_M}x{_N}-gain-mul-softplus"] = dict(M=_M, N=_N, gain=True, mul=True, act=True)
BN_CASES.update({
    "6x48-gain-only": dict(M=6, N=48, gain=True, mul=False, act=False),
    "6x48-mul-only": dict(M=6, N=48, gain=False, mul=True, act=False),
    "6x48-softplus-only": dict(M=6, N=48, gain=False, mul=False, act=True),
    "30x272-one-t": dict(M=30, N=272, gain=True, mul=True, act=True, t=torch.full((30,), 7)),
    "8x48-T3": dict(M=8, N=48, gain=True, mul=False, act=True, T=3, t=torch.tensor([0, 2, 1, 2, 0, 2, 2, 1])),
    "30x272-z-above-20": dict(M=30, N=272, gain=True, mul=True, act=True, beta_shift=24.0),
})


@pytest.mark.parametrize("name", list(BN_CASES))
def test_bn_train_forward_and_backward(name):
    from nested_diffusion_amd import ops
    c = bn_case(**BN_CASES[name])
    r64, r32 = bn_reference(c, torch.float64), bn_reference(c, torch.float32)
    if "z-above-20" in name:
        z = r64["xhat"] * c["gamma"].double() + c["beta"].double()
        assert (z > 20).any() and (z < 20).any()
    d = lambda k: c[k].to(DEV) if k in c else None    # noqa: E731
    t32 = c["t"].to(torch.int32).to(DEV) if "t" in c else None
    act = "softplus" if c["act"] else None
    rm, rv = d("rm"), d("rv")
    out, xhat, rstd = ops.bn_train_forward(d("u"), d("gamma"), d("beta"), table=d("table"), t=t32, mul=d("mul"), act=act, running_mean=rm,
                                           running_var=rv)
    print(f"  {name}")
    for k, got in (("out", out), ("xhat", xhat), ("rstd", rstd), ("rm", rm), ("rv", rv)):
        within(got, r64[k], r32[k], k)
    # the backward reads the forward's own xhat and rstd
    b = ops.bn_train_backward(d("dout"), xhat, rstd, d("gamma"), d("beta"), u=d("u") if "table" in c else None, table=d("table"), t=t32,
                              mul=d("mul"), act=act, want_dmul="mul" in c)
    assert set(b) == {"du", "dgamma", "dbeta"} | ({"dtable"} if "table" in c else set()) | ({"dmul"} if "mul" in c else set())
    for k, got in b.items():
        within(got, r64[k], r32[k], k)
    if "table" in c:
        unused = sorted(set(range(c["T"] + 1)) - set(c["t"].tolist()))
        assert unused and (b["dtable"][unused].cpu() == 0).all() and not torch.signbit(b["dtable"][unused].cpu()).any()
    # without running statistics nothing but the three outputs is written, and the outputs are the same bits
    out2, xhat2, rstd2 = ops.bn_train_forward(d("u"), d("gamma"), d("beta"), table=d("table"), t=t32, mul=d("mul"), act=act)
    assert torch.equal(out, out2) and torch.equal(xhat, xhat2) and torch.equal(rstd, rstd2)


def test_bn_train_refuses_one_row_and_mismatched_arguments():
    from nested_diffusion_amd import ops
    one = torch.zeros(1, 16, device=DEV)
    g = torch.ones(16, device=DEV)
    with pytest.raises(ValueError):
        ops.bn_train_forward(one, g, g)
    with pytest.raises(ValueError):
        ops.bn_train_forward(torch.zeros(129, 16, device=DEV), g, g)
    u = torch.zeros(4, 16, device=DEV)
    with pytest.raises(ValueError):
        ops.bn_train_forward(u, g, g, table=torch.ones(3, 16, device=DEV))                  # a table without t
    with pytest.raises(ValueError):
        ops.bn_train_forward(u, g, g, table=torch.ones(3, 16, device=DEV), t=torch.zeros(4, dtype=torch.int64, device=DEV))   # int64 t
    with pytest.raises(ValueError):
        ops.bn_train_forward(u, g, g, act="relu")


# ---- 2. the sum of squares ------------------------------------------------------------------------------------------------------------------
def sumsq_f32(x, acc=None):
    """the documented order of nd_sumsq on numpy float32 (include/nested_diffusion.h)"""
    x = np.asarray(x, dtype=np.float32).ravel()
    chunks = (x.size + 4095) // 4096
    pad = np.zeros(chunks * 4096, dtype=np.float32)
    pad[:x.size] = x                                   # a skipped element and an added +0 leave the same bits (p >= +0 throughout)
    sq = (pad * pad).reshape(chunks, 16, 256)

    def tree(s):                                       # s[..., 256] -> s[..., 0] after s[j] += s[j + h], h = 128 .. 1
        s = s.copy()
        h = 128
        while h:
            s[..., :h] = s[..., :h] + s[..., h:2 * h]
            h //= 2
        return s[..., 0]

    p = np.zeros((chunks, 256), dtype=np.float32)
    for i in range(16):
        p = p + sq[:, i, :]
    part = tree(p)
    rounds = (chunks + 255) // 256
    pp = np.zeros(rounds * 256, dtype=np.float32)
    pp[:chunks] = part
    q = np.zeros(256, dtype=np.float32)
    for i in range(rounds):
        q = q + pp[i * 256:(i + 1) * 256]
    total = tree(q)
    return np.float32(total) if acc is None else np.float32(acc) + np.float32(total)


@pytest.mark.parametrize("n", [1, 63, 4096, 4097, 1_000_003])
def test_sumsq_is_within_its_chain_bound_and_follows_the_listing(n):
    from nested_diffusion_amd import ops
    x = torch.randn(n, generator=gen(n))
    s64 = float((x.double() ** 2).sum())
    got = ops.sumsq(x.to(DEV))
    L = ops.sumsq_plan(n)["chain"]
    err = abs(float(got) - s64)
    print(f"  n={n}: rel err {err / s64:.3g}, bound {(L + 2) * U:.3g} (chain {L})")
    assert err <= (L + 2) * U * s64
    assert np.float32(float(got)).view(np.uint32) == sumsq_f32(x.numpy()).view(np.uint32)


def test_sumsq_accumulates_over_three_tensors_bit_for_bit():
    from nested_diffusion_amd import ops
    g = gen(3)
    xs = [torch.randn(5000, generator=g), torch.randn(17, 48, generator=g) * 3, torch.randn(1, generator=g)]
    acc = torch.full((), float("nan"), device=DEV)      # the first call overwrites
    want = None
    for i, x in enumerate(xs):
        ops.sumsq(x.to(DEV), acc, accumulate=i > 0)
        want = sumsq_f32(x.numpy(), want)
    assert np.float32(float(acc)).view(np.uint32) == np.float32(want).view(np.uint32)
    img = ops.PackedWeight(xs[1].to(DEV))               # a packed image: the zero padding rows add nothing
    assert float(ops.sumsq(img)) == pytest.approx(float((xs[1].double() ** 2).sum()), rel=64 * U)


# ---- 3. clip + Adam ---------------------------------------------------------------------------------------------------------------------------
def clip_adam_f32(w, m, v, g, a, sumsq, max_norm):
    with np.errstate(all="ignore"):
        g = np.asarray(g, dtype=np.float32)
        if sumsq is not None:
            total = np.sqrt(np.float32(sumsq))
            c = np.float32(max_norm) / (total + np.float32(1e-6))
            coef = c if c < 1 else np.float32(1.0)
            g = g * coef
        return adam_f32(w, m, v, g, a)


CLIP_CASES = {"active": (400.0, 1.0, 1e-3), "inactive": (0.25, 1.0, 1e-3), "null": (None, 1.0, 1e-3), "zero": (0.0, 1.0, 1e-3),
              "inf": (float("inf"), 1.0, 1e-3), "nan": (float("nan"), 1.0, 1e-3), "lr0": (400.0, 1.0, 0.0)}


@pytest.mark.parametrize("name", list(CLIP_CASES))
@pytest.mark.parametrize("n", [1, 1023, 4096])
def test_clip_adam_bit_for_bit(name, n):
    from nested_diffusion_amd import ops
    sumsq, max_norm, lr = CLIP_CASES[name]
    g_ = gen(n)
    w, m, g = (torch.randn(n, generator=g_) for _ in range(3))
    v = torch.rand(n, generator=g_) * 0.1
    a = ops.adam_step(lr, 3)
    want = clip_adam_f32(w.numpy(), m.numpy(), v.numpy(), g.numpy(), a, sumsq, max_norm)
    wd, md, vd = w.to(DEV), m.to(DEV), v.to(DEV)
    ss = None if sumsq is None else torch.tensor(sumsq, dtype=torch.float32, device=DEV)
    ops.clip_adam(wd, md, vd, g.to(DEV), a, sumsq=ss, max_norm=max_norm)
    for got, ref, what in zip((wd, md, vd), want, "wmv"):
        assert np.array_equal(got.cpu().numpy().view(np.uint32), ref.view(np.uint32)), (name, what)
    if name == "active":
        assert not np.array_equal(md.cpu().numpy(), adam_f32(w.numpy(), m.numpy(), v.numpy(), g.numpy(), a)[1])   # the clip did bite


def test_clip_adam_on_a_packed_image_leaves_the_padding_zero():
    from nested_diffusion_amd import ops
    from test_gpu_train_mapping import padding_rows
    N, K = 17, 48
    g_ = gen(5)
    w0, g0 = torch.randn(N, K, generator=g_), torch.randn(N, K, generator=g_)
    w, g = ops.PackedWeight(w0.to(DEV)), ops.PackedWeight(g0.to(DEV))
    m, v = w.zeros_like(), w.zeros_like()
    a = ops.adam_step(1e-3, 1)
    ss = ops.sumsq(g)
    ops.clip_adam(w, m, v, g, a, sumsq=ss, max_norm=1.0)
    want = clip_adam_f32(w0.numpy(), np.zeros((N, K), np.float32), np.zeros((N, K), np.float32), g0.numpy(), a, float(ss), 1.0)
    for img, ref in zip((w, m, v), want):
        assert np.array_equal(img.unpack().cpu().numpy().view(np.uint32), ref.view(np.uint32))
        pad = padding_rows(img).cpu()
        assert pad.numel() == 15 * K and (pad == 0).all()


# ---- 4. the trainer's gradients -------------------------------------------------------------------------------------------------------------
def config_of(B, D, H, Fd, C, T, **optim):
    ns = argparse.Namespace
    return ns(data=ns(dataset="ChestXRay", num_classes=C, label_min_max=[0.001, 0.999]), model=ns(data_dim=D, hidden_dim=H, feature_dim=Fd, arch="linear"),
              diffusion=ns(timesteps=T, beta_schedule="linear", beta_start=1e-4, beta_end=0.02, aux_cls=ns(arch="sevit"), include_guidance=True,
                           trained_aux_cls_ckpt_path="", trained_diffusion_ckpt_path=[[]]),
              optim=ns(optimizer="Adam", lr=1e-3, beta1=0.9, eps=1e-8, weight_decay=0.0, amsgrad=False, grad_clip=1.0, lr_schedule=True, min_lr=0.0,
                       **optim),
              training=ns(batch_size=B, n_epochs=2, warmup_epochs=1, validation_freq=1, logging_freq=0), testing=ns(batch_size=B))


ENC_BIAS = {"encoder_x.0.bias": "encoder_x.0", "encoder_x.3.bias": "encoder_x.3", "encoder_x.6.bias": "encoder_x.6"}


@pytest.mark.parametrize("dims", [(6, 48, 32, 32, 2, 10), (30, 2048, 256, 256, 2, 100), (2, 16, 16, 16, 1, 3)], ids=str)
def test_trainer_gradients_against_the_float64_oracle(dims):
    from nested_diffusion_amd.train_diffusion import PARAM_KEYS, NoiseEstimatorTrainer
    B, D, H, Fd, C, T = dims
    state = oracle_mod.random_state(D, H, Fd, C, T, seed=11)
    batch = oracle_mod.random_batch(B, D, C, T, seed=12)
    tr = NoiseEstimatorTrainer(config_of(*dims), DEV, state_dict=state)
    o = {d: oracle_mod.Oracle(state, tr.alphas_bar_sqrt, tr.one_minus_alphas_bar_sqrt, dtype=d) for d in (torch.float32, torch.float64)}
    l64, l32 = o[torch.float64].backward(*batch), o[torch.float32].backward(*batch)
    g64, g32 = o[torch.float64].grads(), o[torch.float32].grads()
    x, y0, yhat, t, e = batch
    loss, g = tr.gradients(x.to(DEV), y0.to(DEV), yhat.to(DEV), t, e.to(DEV))
    print(f"  dims {dims}")
    within(loss, l64, l32, "loss")
    assert tuple(g) == PARAM_KEYS and len(g) == 29
    for k in PARAM_KEYS:
        assert tuple(g[k].shape) == tuple(g64[k].shape), k
        extra = 0.0
        if k in ENC_BIAS:      # the true gradient is 0 (BatchNorm removes a bias): what is left is the rounding of a B-term column sum of du
            extra = (B + 2) * 2.0 ** -23 * float(o[torch.float64].du[ENC_BIAS[k]].abs().sum(0).max())
        within(g[k], g64[k], g32[k], k, extra)


# ---- 5. one step, bit for bit given the GPU's own gradients ---------------------------------------------------------------------------------
def test_step_is_the_listing_on_the_trainers_own_gradients():
    from nested_diffusion_amd import ops
    from nested_diffusion_amd.train_diffusion import LIN1_K, PARAM_KEYS, NoiseEstimatorTrainer
    dims = (6, 48, 32, 32, 2, 10)
    B, D, H, Fd, C, T = dims
    tr = NoiseEstimatorTrainer(config_of(*dims), DEV, seed=3)
    sd0 = tr.state_dict()
    assert float(sd0["norm.weight"].min()) == 1.0 and float(sd0["norm.bias"].abs().max()) == 0.0 and int(sd0["norm.num_batches_tracked"]) == 0
    assert float(sd0["lin2.embed.weight"].min()) >= 0.0 and tuple(sd0["lin2.embed.weight"].shape) == (T + 1, Fd)
    assert float(sd0["encoder_x.0.weight"].abs().max()) <= 1.0 / np.sqrt(D) and float(sd0["lin1.lin.weight"].abs().max()) <= 1.0 / np.sqrt(2 * C)
    for s in range(2):                                 # the second step starts from non-zero moments
        x, y0, yhat, t, e = oracle_mod.random_batch(B, D, C, T, seed=20 + s)
        args = (x.to(DEV), y0.to(DEV), yhat.to(DEV), t, e.to(DEV))
        before = {w: {k: q.cpu().numpy() for k, q in tr.tensors(w).items()} for w in "pmv"}
        loss_g, g = tr.gradients(*args)
        g = {k: q.cpu().numpy() for k, q in g.items()}
        g["lin1.lin.weight"] = np.concatenate([g["lin1.lin.weight"], np.zeros((Fd, LIN1_K - 2 * C), np.float32)], axis=1)
        tr.lr = 1e-3 * (s + 1)
        loss, norm = tr.step(*args)
        assert torch.equal(loss, loss_g)
        ss = float(tr.last_sumsq)
        assert float(norm) == float(np.sqrt(np.float32(ss)))
        host_ss = sum(float((q.astype(np.float64) ** 2).sum()) for q in g.values())
        assert abs(ss - host_ss) <= 64 * U * host_ss    # 29 tensors, chains of at most 34 additions each
        a = ops.adam_step(tr.lr, s + 1)
        after = {w: {k: q.cpu().numpy() for k, q in tr.tensors(w).items()} for w in "pmv"}
        for k in PARAM_KEYS:
            want = clip_adam_f32(before["p"][k], before["m"][k], before["v"][k], g[k], a, ss, 1.0)
            for w, ref in zip("pmv", want):
                assert np.array_equal(after[w][k].view(np.uint32), ref.view(np.uint32)), (s, k, w)
        for w in "pmv":
            pad = after[w]["lin1.lin.weight"][:, 2 * C:]
            assert pad.shape == (Fd, LIN1_K - 2 * C) and (pad == 0).all()
        assert int(tr.state_dict()["unetnorm3.num_batches_tracked"]) == s + 1
        assert tr.state_dict()["norm.num_batches_tracked"].dtype == torch.int64


# ---- 6. five steps against the reference's recorded results ---------------------------------------------------------------------------------
LOOSE = ("encoder_x.0.bias", "encoder_x.3.bias", "encoder_x.6.bias", "encoder_x.1.running_mean", "encoder_x.4.running_mean", "norm.running_mean")


@pytest.fixture(scope="module")
def fixture_and_yardsticks():
    fx = oracle_mod.load_fixture()
    return fx, {p: oracle_mod.fixture_run(fx, torch.float64, p) for p in ("", "noclip/")}


@pytest.mark.parametrize("prefix", ["", "noclip/"])
def test_five_steps_reproduce_the_reference(fixture_and_yardsticks, prefix):
    """Everything within 8 x the deviation of the float64 oracle from the reference's fp32 results (the reference's own fp32 error),
    per quantity.  The three encoder biases and the running means behind them are left out: their true gradient is 0, Adam turns the
    rounding noise there into lr-sized steps of arbitrary sign, and BatchNorm removes them from the output again."""
    from nested_diffusion_amd.engine import EnsembleEngine
    from nested_diffusion_amd.train_diffusion import NoiseEstimatorTrainer
    fx, yard = fixture_and_yardsticks
    r64 = yard[prefix]
    B, D, H, Fd, C, T, eval_t = (int(v) for v in fx["dims"])
    tr = NoiseEstimatorTrainer(config_of(B, D, H, Fd, C, T, ), DEV, state_dict=oracle_mod.fixture_state(fx, "init/"))
    tr.grad_clip = 1e9 if prefix else 1.0
    for mine, name in ((tr.alphas_bar_sqrt, "alphas_bar_sqrt"), (tr.one_minus_alphas_bar_sqrt, "one_minus_alphas_bar_sqrt")):
        # the trainer's own schedule tables, from this host's torch (cumprod and sqrt of values below 1: an ulp of 1 is 2^-23)
        assert float((mine - torch.from_numpy(fx[name])).abs().max()) <= 2.0 ** -23, name
    print(f"  run {prefix!r}")
    # one deviation per kind of quantity: the largest over the five steps (a single step's can be next to 0 by chance)
    own = {what: float(np.abs(np.array(r64[what]) - fx[prefix + what].astype(np.float64)).max()) for what in ("loss", "norm")}
    for s in range(fx["x"].shape[0]):
        x, yhat, e = (torch.from_numpy(fx[k][s]).to(DEV) for k in ("x", "yhat", "e"))
        y0 = F.one_hot(torch.from_numpy(fx["labels"][s]), num_classes=C).float().to(DEV)
        loss, norm = tr.step(x, y0, yhat, torch.from_numpy(fx["t"][s]), e)
        for what, got in (("loss", loss), ("norm", norm)):
            ref = float(fx[prefix + what][s])
            dev64 = own[what]
            err = abs(float(got) - ref)
            print(f"    step {s} {what}: err {err:.3g}, reference's own {dev64:.3g}")
            assert err <= 8 * dev64, (s, what, err, dev64)
    sd = tr.state_dict()
    for k, got in sd.items():
        if k.endswith("num_batches_tracked"):
            assert int(got) == 5 and got.dtype == torch.int64
            continue
        ref = torch.from_numpy(fx[prefix + "final/" + k])
        assert tuple(got.shape) == tuple(ref.shape), k
        if k in LOOSE:
            continue
        dev64 = float((r64["final"][k].double() - ref.double()).abs().max())
        err = float((got.double() - ref.double()).abs().max())
        print(f"    final {k}: err {err:.3g}, reference's own {dev64:.3g}")
        assert err <= 8 * dev64, (k, err, dev64)
    eng = EnsembleEngine(C, D, H, Fd, T, n_members=1, max_batch=B, device=DEV)
    eng.load_member(0, sd)
    eng.encode(x)
    out = eng.eps_theta(0, torch.from_numpy(fx[prefix + "eval_y"]), yhat, eval_t).cpu()
    ref = torch.from_numpy(fx[prefix + "eval_out"])
    dev64 = float((r64["eval_out"].double() - ref.double()).abs().max())
    err = float((out.double() - ref.double()).abs().max())
    print(f"    eval output: err {err:.3g}, reference's own {dev64:.3g}")
    assert err <= 8 * dev64


# ---- 7. Diffusion.train end to end ----------------------------------------------------------------------------------------------------------
def test_diffusion_train_end_to_end_on_synthetic_data(tmp_path):
    from nested_diffusion_amd.data import SyntheticLoader
    from nested_diffusion_amd.mapping import Classifier, GuidingConditioner, VisionTransformer
    from nested_diffusion_amd.runner import Diffusion
    embed, heads, depth, img, patch, K = 128, 2, 2, 32, 16, 2
    B, D, H, Fd, C, T = 6, 3 * img * img, 32, 32, 2, 5
    vp = ref_cpu.init_vit_params(embed=embed, depth=depth, patch=patch, img=img, seed=5)
    mlps = [ref_cpu.init_classifier_params((img // patch) ** 2 * embed, widths=(64, 32, 16), seed=10 + i) for i in range(K)]
    cond = GuidingConditioner(VisionTransformer(vp, heads), [Classifier(m) for m in mlps])
    cfg = config_of(B, D, H, Fd, C, T)
    args = argparse.Namespace(seed=7, mc_trials=2, log_path=str(tmp_path), preprocess="grayscaled")
    runner = Diffusion(args, cfg, device=DEV, conditioner=cond)
    res = runner.train(1, train_loader=SyntheticLoader(3, B, C, seed=1, size=img), valid_loader=SyntheticLoader(2, B, C, seed=2, size=img))
    assert len(res["losses"]) == 2 and all(np.isfinite(v) for v in res["losses"])
    assert sorted(res["accuracies"]) == [0, 1]
    files = glob.glob(os.path.join(str(tmp_path), "diffu1_ckpt_best_eph*_acc*.pth"))
    assert files and res["best"] in files
    assert re.fullmatch(r"diffu1_ckpt_best_eph[01]_acc\d+\.\d{4}\.pth", os.path.basename(res["best"]))
    ck = torch.load(res["best"])
    assert set(ck) == {"noise_estimator", "optimizer", "epoch"} and set(ck["optimizer"]) == {"step", "lr"}
    assert set(ck["noise_estimator"]) == set(ref_cpu.init_cond_model_params(16, 16, 16, C, T))
    # the checkpoint is what load_noise_estimators reads, and predict_batch runs on it
    cfg.diffusion.trained_diffusion_ckpt_path = [[res["best"]]]
    r2 = Diffusion(args, cfg, device=DEV, conditioner=cond)
    r2.load_noise_estimators(max_batch=B)
    assert r2.members == [0]
    out = r2.predict_batch(torch.rand(B, 3, img, img, generator=gen(9)).to(DEV))
    assert tuple(out["prob"].shape) == (B, C) and torch.isfinite(out["prob"]).all()
    with pytest.raises(NotImplementedError):
        runner.train(K)
