"""The EMA shadow of the noise estimators on the GPU: nd_clip_adam_ema bit for bit against the float32 listing that
tests/test_ema_host.py pins to the reference's EMA class, on tensors and packed images; ops.clip_adam's refusals; the trainer with a
shadow beside one without (same bits in everything else, the shadow equal to the listing on the trainer's own parameters); snapshots;
and Diffusion.train with --ema / a runner with --use_ema end to end.

The trainer test is deliberately not another five-step replay against diffusion_train.npz: the shadow is a deterministic function of the
parameter trajectory, which test_gpu_diffusion_train.py already pins, and the listing is pinned to the reference by tests/golden/ema.npz."""
import argparse
import os
import shutil

import numpy as np
import pytest
import torch

import _diffusion_train_oracle as oracle_mod
from oracle import ref_cpu
from test_ema_host import differing, ema_contracted, ema_f32, ema_wrong_one_minus_mu, same_bits
from test_gpu_diffusion_train import CLIP_CASES, config_of
from test_gpu_resume import Preempted, same_state

pytestmark = pytest.mark.gpu
DEV = "cuda"
RATES = [0.9999, 0.5]
FLT_MAX, FLT_MIN = float(np.finfo(np.float32).max), float(np.finfo(np.float32).tiny)
# the fixture's special values: signed zeros, infinities, NaN, denormals, a normal whose product with 1e-4 is denormal, the extremes
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-40, -1e-40, 1.4e-45, 5e-35, -5e-35, FLT_MIN, -FLT_MIN, FLT_MAX, -FLT_MAX, 1.0,
                     -1e-4], dtype=np.float64).astype(np.float32)
GRID_FLOATS = 16384 * 256 * 4                                   # what the float4 path's largest grid covers in one sweep
SIZES = {"1": 1, "3": 3, "4": 4, "1023": 1023, "4096": 4096, "4096-offset": 4096, "wrap-vec": GRID_FLOATS + 4 * 100_003,
         "wrap-scalar": GRID_FLOATS // 4 + 100_003}


def bits(t):
    return t.contiguous().view(torch.int32)


def make_case(n, seed, offset):
    """(w, m, v, g, s) on the device.  The ordinary weights change scale along the tensor, so that (1 - mu) * w and mu * s are often
    of one magnitude (where a contracted multiply-add shows); the head of w and s holds every pair of SPECIALS (as many as fit), with
    m = g = 0 there so that Adam leaves exactly that w: m stays 0, m / denom = 0, w - step * 0 = w."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    k = n + 1 if offset else n
    bufs = [torch.randn(k, generator=gen, device=DEV) for _ in range(4)] + [torch.rand(k, generator=gen, device=DEV) * 0.1]
    w, m, g, s, v = ([b[1:] for b in bufs] if offset else bufs)
    scale = torch.tensor([1.0, 3.0e3, 1.0e4, 1.0e-3, 30.0], device=DEV).repeat(n // 5 + 1)[:n]
    w.mul_(scale)
    sp = torch.from_numpy(SPECIALS)
    pairs_w, pairs_s = sp.repeat_interleave(len(sp)), sp.repeat(len(sp))
    if n < 64:                                                   # a few pairs that differ from seed to seed
        pick = (torch.arange(n) * 37 + seed * 11) % len(pairs_w)
        pairs_w, pairs_s = pairs_w[pick], pairs_s[pick]
    c = min(n, len(pairs_w))
    w[:c], s[:c] = pairs_w[:c].to(DEV), pairs_s[:c].to(DEV)
    m[:c], g[:c] = 0.0, 0.0
    return w, m, v, g, s


# ---- 1. the kernel, bit for bit ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mu", RATES)
@pytest.mark.parametrize("name", list(CLIP_CASES))
@pytest.mark.parametrize("size", list(SIZES))
def test_clip_adam_ema_bit_for_bit(size, name, mu):
    from nested_diffusion_amd import ops
    n, offset = SIZES[size], size.endswith("offset")
    sumsq, max_norm, lr = CLIP_CASES[name]
    w, m, v, g, s = make_case(n, seed=n % 1000 + len(name), offset=offset)
    if offset:
        assert n % 4 == 0 and w.data_ptr() % 16 == 4             # the scalar path although n is a multiple of four
    if size.startswith("wrap"):
        per_sweep = GRID_FLOATS if size == "wrap-vec" else GRID_FLOATS // 4
        assert n > per_sweep and (n - per_sweep) % (per_sweep // 16384) != 0 and (n % 4 == 0) == (size == "wrap-vec")
    a, e = ops.adam_step(lr, 3), ops.ema_step(mu)
    ss = None if sumsq is None else torch.tensor(sumsq, dtype=torch.float32, device=DEV)
    w0, m0, v0 = w.clone(), m.clone(), v.clone()
    before = w.cpu().numpy()
    ops.clip_adam(w0, m0, v0, g, a, sumsq=ss, max_norm=max_norm)
    s_old, g_old = s.cpu().numpy(), g.clone()
    ops.clip_adam(w, m, v, g, a, sumsq=ss, max_norm=max_norm, shadow=s, ema=e)
    for got, ref, what in ((w, w0, "w"), (m, m0, "m"), (v, v0, "v"), (g, g_old, "g")):       # the existing listing is untouched
        assert torch.equal(bits(got), bits(ref)), (size, name, what)
    w_new = w.cpu().numpy()
    c = min(n, len(SPECIALS) ** 2)
    assert same_bits(w_new[:c], before[:c])                      # the special weights came through Adam unchanged (NaN stays NaN)
    want = ema_f32(w_new, s_old, mu)
    got = s.cpu().numpy()
    assert same_bits(got, want), (size, name, mu, differing(got, want))
    if n >= 1023 and mu == 0.9999:                               # the data can tell both mistakes from the listing
        assert differing(ema_wrong_one_minus_mu(w_new, s_old, mu), want) > 0
        assert differing(ema_contracted(w_new, s_old, mu, 0), want) > 0 and differing(ema_contracted(w_new, s_old, mu, 1), want) > 0


# ---- 2. packed images ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mu", RATES)
def test_clip_adam_ema_on_a_packed_image_leaves_the_padding_zero(mu):
    from nested_diffusion_amd import ops
    from test_gpu_train_mapping import padding_rows
    N, K = 17, 48
    gen = torch.Generator().manual_seed(5)
    w0, g0, s0 = (torch.randn(N, K, generator=gen) for _ in range(3))
    w, g, s = (ops.PackedWeight(t.to(DEV)) for t in (w0, g0, s0))
    m, v = w.zeros_like(), w.zeros_like()
    w1, g1 = ops.PackedWeight(w0.to(DEV)), ops.PackedWeight(g0.to(DEV))
    m1, v1 = w1.zeros_like(), w1.zeros_like()
    a, e = ops.adam_step(1e-3, 1), ops.ema_step(mu)
    ss = ops.sumsq(g)
    ops.clip_adam(w1, m1, v1, g1, a, sumsq=ss, max_norm=1.0)
    ops.clip_adam(w, m, v, g, a, sumsq=ss, max_norm=1.0, shadow=s, ema=e)
    for img, ref in ((w, w1), (m, m1), (v, v1)):
        assert torch.equal(bits(img.data), bits(ref.data))
    want = ema_f32(w.unpack().cpu().numpy(), s0.numpy(), mu)
    assert same_bits(s.unpack().cpu().numpy(), want)
    for img in (w, m, v, s):
        pad = padding_rows(img).cpu()
        assert pad.numel() == 15 * K and (pad == 0).all()


# ---- 3. the refusals of ops.clip_adam ---------------------------------------------------------------------------------------------------------
def test_clip_adam_refuses_a_shadow_it_cannot_take():
    from nested_diffusion_amd import _lib, ops
    a, e = ops.adam_step(1e-3, 1), ops.ema_step(0.9)
    w, m, v, g, s = (torch.randn(8, 16, device=DEV) for _ in range(5))
    keep = [t.clone() for t in (w, m, v, s)]
    with pytest.raises(ValueError, match="come together"):
        ops.clip_adam(w, m, v, g, a, shadow=s)
    with pytest.raises(ValueError, match="come together"):
        ops.clip_adam(w, m, v, g, a, ema=e)
    with pytest.raises(ValueError, match="distinct"):
        ops.clip_adam(w, m, v, g, a, shadow=w, ema=e)
    with pytest.raises(ValueError, match="distinct"):
        ops.clip_adam(w, m, v, g, a, shadow=g, ema=e)
    with pytest.raises(ValueError):
        ops.clip_adam(w, m, v, g, a, shadow=torch.randn(16, 8, device=DEV), ema=e)
    with pytest.raises(_lib.NdError, match="shadow must be torch.float32"):
        ops.clip_adam(w, m, v, g, a, shadow=torch.randn(8, 16, device=DEV).double(), ema=e)
    with pytest.raises(_lib.NdError, match="shadow must be a GPU tensor"):
        ops.clip_adam(w, m, v, g, a, shadow=s.cpu(), ema=e)
    with pytest.raises(ValueError, match="contiguous"):
        ops.clip_adam(w, m, v, g, a, shadow=torch.randn(16, 8, device=DEV).t(), ema=e)
    pw, pg = ops.PackedWeight(w), ops.PackedWeight(g)
    pm, pv = pw.zeros_like(), pw.zeros_like()
    with pytest.raises(ValueError, match="shadow"):                                # a tensor beside four images, and the reverse
        ops.clip_adam(pw, pm, pv, pg, a, shadow=s, ema=e)
    with pytest.raises(ValueError, match="shadow"):
        ops.clip_adam(w, m, v, g, a, shadow=pw.zeros_like(), ema=e)
    with pytest.raises(ValueError, match="shadow"):                                # an image of another shape
        ops.clip_adam(pw, pm, pv, pg, a, shadow=ops.PackedWeight(torch.randn(8, 32, device=DEV)), ema=e)
    with pytest.raises(ValueError, match="distinct"):
        ops.clip_adam(pw, pm, pv, pg, a, shadow=pm, ema=e)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError):
            ops.clip_adam(w, m, v, g, a, shadow=s.to("cuda:1"), ema=e)
    for t, k in zip((w, m, v, s), keep):                                           # nothing ran
        assert torch.equal(t, k)


# ---- 4. the trainer -----------------------------------------------------------------------------------------------------------------------
DIMS = (6, 48, 32, 32, 2, 10)


def batch_on_device(seed):
    B, D, H, Fd, C, T = DIMS
    x, y0, yhat, t, e = oracle_mod.random_batch(B, D, C, T, seed=seed)
    return x.to(DEV), y0.to(DEV), yhat.to(DEV), t, e.to(DEV)


def host(tensors):
    return {k: q.cpu().numpy() for k, q in tensors.items()}


@pytest.mark.parametrize("mu", [0.9, 0.9999])
def test_trainer_with_a_shadow_moves_everything_else_as_one_without(mu):
    from nested_diffusion_amd.train_diffusion import LIN1_K, PARAM_KEYS, NoiseEstimatorTrainer
    B, D, H, Fd, C, T = DIMS
    plain = NoiseEstimatorTrainer(config_of(*DIMS), DEV, seed=3)
    tr = NoiseEstimatorTrainer(config_of(*DIMS), DEV, seed=3, ema_rate=mu)
    assert plain.shadow is None and plain.ema_rate is None and "ema" not in plain.training_state()
    assert "ema_rate" not in plain.training_state()["meta"]
    with pytest.raises(ValueError, match="no EMA shadow"):
        plain.ema_state_dict()
    shadow, p = host(tr.tensors("ema")), host(tr.tensors("p"))
    assert tuple(shadow) == PARAM_KEYS and len(shadow) == 29
    for k in PARAM_KEYS:                                         # EMA.register: a clone of every parameter, in another buffer
        assert same_bits(shadow[k], p[k]), k
        q, s = tr.p[k], tr.shadow[k]
        assert type(q) is type(s) and (q.data if hasattr(q, "N") else q).data_ptr() != (s.data if hasattr(s, "N") else s).data_ptr()
    for step in range(3):
        args = batch_on_device(30 + step)
        plain.lr = tr.lr = 1e-3 * (step + 1)
        loss0, norm0 = plain.step(*args)
        loss1, norm1 = tr.step(*args)
        assert torch.equal(bits(loss0), bits(loss1)) and torch.equal(bits(norm0), bits(norm1))
        for which in "pmv":
            a, b = plain.tensors(which), tr.tensors(which)
            for k in PARAM_KEYS:
                assert torch.equal(bits(a[k]), bits(b[k])), (step, which, k)
        for k, b in plain.buf.items():
            assert torch.equal(bits(b), bits(tr.buf[k])), (step, k)
        p, after = host(tr.tensors("p")), host(tr.tensors("ema"))
        n_moved = 0
        for k in PARAM_KEYS:
            want = ema_f32(p[k], shadow[k], mu)
            assert same_bits(after[k], want), (step, k, differing(after[k], want))
            n_moved += differing(after[k], p[k])
        assert n_moved > 0                                       # the shadow lags behind the weights
        pad = after["lin1.lin.weight"][:, 2 * C:]
        assert pad.shape == (Fd, LIN1_K - 2 * C) and (pad == 0).all()
        shadow = after
    sd, esd = tr.state_dict(), tr.ema_state_dict()
    assert list(esd) == list(sd) and len(sd) == 29 + 18
    for k in sd:
        assert esd[k].dtype == sd[k].dtype and tuple(esd[k].shape) == tuple(sd[k].shape) and esd[k].device.type == "cpu", k
        if k in PARAM_KEYS:
            full = shadow[k][:, :2 * C] if k == "lin1.lin.weight" else shadow[k]
            assert same_bits(esd[k].numpy(), full), k
        else:                                                    # the LIVE running statistics and counters
            assert torch.equal(esd[k], sd[k]), k
    assert int(esd["norm.num_batches_tracked"]) == 3 and esd["norm.num_batches_tracked"].dtype == torch.int64
    assert not torch.equal(esd["lin4.weight"], sd["lin4.weight"])
    assert torch.equal(plain.state_dict()["lin4.weight"], sd["lin4.weight"])
    assert tr.ema_state_dict(cpu=False)["lin4.weight"].device.type == "cuda"


# ---- 5. snapshots -------------------------------------------------------------------------------------------------------------------------
def test_snapshot_carries_the_shadow_and_mismatches_are_refused_by_name():
    from nested_diffusion_amd.train_diffusion import NoiseEstimatorTrainer
    mu = 0.9
    a = NoiseEstimatorTrainer(config_of(*DIMS), DEV, seed=3, ema_rate=mu)
    for step in range(2):
        a.step(*batch_on_device(40 + step))
    state = a.training_state()
    assert state["meta"]["ema_rate"] == mu and sorted(state["ema"]) == sorted(state["p"])
    for k in state["p"]:
        assert state["ema"][k].shape == state["p"][k].shape and state["ema"][k].device.type == "cpu"
    assert any(not torch.equal(state["ema"][k], state["p"][k]) for k in state["p"])
    b = NoiseEstimatorTrainer(config_of(*DIMS), DEV, seed=99, ema_rate=mu)
    b.load_training_state(state)
    assert same_state(b.training_state(), state) == 4 * 29 + 12
    args = batch_on_device(42)
    la, lb = a.step(*args), b.step(*args)
    assert torch.equal(bits(la[0]), bits(lb[0])) and torch.equal(bits(la[1]), bits(lb[1]))
    assert same_state(a.training_state(), b.training_state()) == 4 * 29 + 12
    # the refusals, each before any tensor of the trainer is replaced
    plain = NoiseEstimatorTrainer(config_of(*DIMS), DEV, seed=5)
    other = NoiseEstimatorTrainer(config_of(*DIMS), DEV, seed=5, ema_rate=0.5)
    with_ema = NoiseEstimatorTrainer(config_of(*DIMS), DEV, seed=5, ema_rate=mu)
    plain_state = plain.training_state()
    headless = dict(state, meta={k: v for k, v in state["meta"].items() if k != "ema_rate"})        # holds 'ema', records no rate
    for tr, snap, words in ((plain, state, "this run has none"), (plain, headless, "holds an EMA shadow"),
                            (with_ema, plain_state, "does not record it"), (other, state, "0.9")):
        before = tr.training_state()
        with pytest.raises(ValueError, match="ema_rate") as err:
            tr.load_training_state(snap)
        assert words in str(err.value)
        assert same_state(tr.training_state(), before) > 0


# ---- 6. Diffusion.train and the readers, end to end -------------------------------------------------------------------------------------------
E2E = dict(embed=128, heads=2, depth=2, img=32, patch=16, K=2, B=6, H=32, F=32, C=2, T=5)


class StoppingSynthetic:
    """data.SyntheticLoader that raises Preempted instead of starting its (stop_after + 1)-th pass"""

    def __init__(self, inner, stop_after=None):
        self.inner, self.stop_after, self.passes = inner, stop_after, 0
        self.global_batch = inner.global_batch

    def __len__(self):
        return len(self.inner)

    def __iter__(self):
        if self.passes == self.stop_after:
            raise Preempted()
        self.passes += 1
        return iter(self.inner)


@pytest.fixture(scope="module")
def conditioner():
    from nested_diffusion_amd.mapping import Classifier, GuidingConditioner, VisionTransformer
    c = E2E
    vp = ref_cpu.init_vit_params(embed=c["embed"], depth=c["depth"], patch=c["patch"], img=c["img"], seed=5)
    mlps = [ref_cpu.init_classifier_params((c["img"] // c["patch"]) ** 2 * c["embed"], widths=(64, 32, 16), seed=10 + i) for i in range(c["K"])]
    return GuidingConditioner(VisionTransformer(vp, c["heads"]), [Classifier(m) for m in mlps])


def e2e_config(paths=None):
    c = E2E
    cfg = config_of(c["B"], 3 * c["img"] * c["img"], c["H"], c["F"], c["C"], c["T"])
    cfg.model.ema, cfg.model.ema_rate = True, 0.5                # a rate at which the shadow visibly differs after six steps
    if paths is not None:
        cfg.diffusion.trained_diffusion_ckpt_path = [paths]
    return cfg


def e2e_train(conditioner, log_dir, stop_after=None, **flags):
    from nested_diffusion_amd.data import SyntheticLoader
    from nested_diffusion_amd.runner import Diffusion
    c = E2E
    os.makedirs(log_dir, exist_ok=True)
    args = argparse.Namespace(seed=7, mc_trials=2, log_path=log_dir, preprocess="grayscaled", **flags)
    runner = Diffusion(args, e2e_config(), device=DEV, conditioner=conditioner)
    train = StoppingSynthetic(SyntheticLoader(3, c["B"], c["C"], seed=1, size=c["img"]), stop_after)
    try:
        return runner.train(1, train_loader=train, valid_loader=SyntheticLoader(2, c["B"], c["C"], seed=2, size=c["img"])), runner
    except Preempted:
        return None, runner


@pytest.fixture(scope="module")
def e2e_runs(conditioner, tmp_path_factory):
    root = tmp_path_factory.mktemp("ema_e2e")
    plain, run_plain = e2e_train(conditioner, str(root / "plain"))
    ema, run_ema = e2e_train(conditioner, str(root / "ema"), ema=True)
    return {"root": root, "plain": plain, "ema": ema, "run_plain": run_plain, "run_ema": run_ema}


def test_train_with_the_flag_writes_the_same_live_weights_and_a_fourth_entry(e2e_runs):
    plain, ema = e2e_runs["plain"], e2e_runs["ema"]
    assert e2e_runs["run_plain"].trainer.shadow is None          # model.ema: True in the config, no flag: no shadow
    assert e2e_runs["run_ema"].trainer.ema_rate == 0.5
    assert plain["losses"] == ema["losses"] and len(plain["losses"]) == 2 and all(np.isfinite(v) for v in plain["losses"])
    assert plain["accuracies"] == ema["accuracies"] and sorted(plain["accuracies"]) == [0, 1]
    assert plain["best"] is not None and os.path.basename(plain["best"]) == os.path.basename(ema["best"])
    ck0, ck1 = torch.load(plain["best"]), torch.load(ema["best"])
    assert set(ck0) == {"noise_estimator", "optimizer", "epoch"}
    assert set(ck1) == {"noise_estimator", "optimizer", "epoch", "ema"}
    assert ck0["optimizer"] == ck1["optimizer"] and ck0["epoch"] == ck1["epoch"]
    assert list(ck0["noise_estimator"]) == list(ck1["noise_estimator"]) == list(ck1["ema"])
    for k, t in ck0["noise_estimator"].items():
        assert t.dtype == ck1["noise_estimator"][k].dtype and same_bits_t(t, ck1["noise_estimator"][k]), k
        assert ck1["ema"][k].dtype == t.dtype and tuple(ck1["ema"][k].shape) == tuple(t.shape), k
    assert same_bits_t(ck1["ema"]["norm.running_mean"], ck1["noise_estimator"]["norm.running_mean"])
    assert not torch.equal(ck1["ema"]["lin4.weight"], ck1["noise_estimator"]["lin4.weight"])
    assert not os.path.exists(os.path.join(str(e2e_runs["root"] / "ema"), "ckpt.pth"))


def same_bits_t(a, b):
    if not a.dtype.is_floating_point:
        return torch.equal(a, b)
    return same_bits(a.numpy(), b.numpy())


def test_a_runner_with_use_ema_samples_from_the_shadow(e2e_runs, conditioner):
    from nested_diffusion_amd.runner import Diffusion
    c = E2E
    best = e2e_runs["ema"]["best"]
    ck = torch.load(best)
    x = torch.rand(c["B"], 3, c["img"], c["img"], generator=torch.Generator().manual_seed(9)).to(DEV)

    def predict(states=None, **flags):
        args = argparse.Namespace(seed=7, mc_trials=2, log_path=str(e2e_runs["root"]), preprocess="grayscaled", **flags)
        r = Diffusion(args, e2e_config([best]), device=DEV, conditioner=conditioner, noise_estimator_states=states)
        r.load_noise_estimators(max_batch=c["B"])
        assert r.members == [0]
        return r.predict_batch(x)

    live, shadow, injected = predict(), predict(use_ema=True), predict(states=[ck["ema"]])
    for key in ("prob", "samples"):
        assert torch.isfinite(shadow[key]).all()
        assert torch.equal(bits(shadow[key]), bits(injected[key])), key
    assert tuple(shadow["prob"].shape) == (c["B"], c["C"])
    assert not torch.equal(shadow["samples"], live["samples"])
    # a checkpoint written without --ema is refused by name
    r = Diffusion(argparse.Namespace(seed=7, mc_trials=2, use_ema=True), e2e_config([e2e_runs["plain"]["best"]]), device=DEV,
                  conditioner=conditioner)
    with pytest.raises(KeyError) as err:
        r.load_noise_estimators(max_batch=c["B"])
    assert e2e_runs["plain"]["best"] in str(err.value) and "--use_ema" in str(err.value)


def test_an_interrupted_run_resumes_to_the_same_shadow(e2e_runs, conditioner):
    root = e2e_runs["root"]
    half, run_h = e2e_train(conditioner, str(root / "half"), stop_after=1, ema=True, snapshot_epochs=1)
    assert half is None and run_h.trainer.t == 3
    snap = torch.load(str(root / "half" / "ckpt.pth"))
    assert snap["loop"]["next_epoch"] == 1 and snap["trainer"]["meta"]["ema_rate"] == 0.5 and len(snap["trainer"]["ema"]) == 29
    torch.manual_seed(12345)                                     # the generators the loop draws from, moved on purpose
    torch.rand(3)
    torch.rand(3, device=DEV)
    res, run_c = e2e_train(conditioner, str(root / "half"), ema=True, snapshot_epochs=1, resume_training=True)
    straight = e2e_runs["run_ema"].trainer
    assert res["losses"] == e2e_runs["ema"]["losses"] and res["accuracies"] == e2e_runs["ema"]["accuracies"]
    assert os.path.basename(res["best"]) == os.path.basename(e2e_runs["ema"]["best"])
    a, b = straight.tensors("ema"), run_c.trainer.tensors("ema")
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), k
    assert same_state(run_c.trainer.training_state(), straight.training_state()) == 4 * 29 + 12
    for k, t in torch.load(res["best"])["ema"].items():
        assert same_bits_t(t, torch.load(e2e_runs["ema"]["best"])["ema"][k]), k
    # a resume without the flag is refused by name, and so is one that asks for a shadow the snapshot does not hold
    shutil.copytree(str(root / "half"), str(root / "noflag"))
    with pytest.raises(ValueError, match="ema_rate"):
        e2e_train(conditioner, str(root / "noflag"), snapshot_epochs=1, resume_training=True)
