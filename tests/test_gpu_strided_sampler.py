"""Sampler plans on the GPU (nd_set_sampler: strided timesteps, generalized eta update): whole trajectories against a test-side oracle,
the bit-level claims (eager == graph, no stale graph, many-rows head == per-row head, device-table path == by-value path, eta = 0 reads no
draw past the first, a cleared plan is the default path), nd_predict_batch under a plan, the stateful refusals and the input gradient
through a strided chain.

The oracle is a loop in this file: ref_cpu.encoder_x and ref_cpu.trunk in fp32 (the noise estimator is not what is under test), the update
in float64 from the formulas of include/nested_diffusion.h ("SAMPLER PLAN") restated in test_strided_sampler_host.coef64 -- not from
diffusion_utils.sampler_plan.  Criterion: the project's own for a trajectory, |got - ref| <= 5e-5 * max(1, |ref|max)."""
import argparse
import ctypes as C
import types

import pytest
import torch

from oracle import ref_cpu
from test_strided_sampler_host import coef64

pytestmark = pytest.mark.gpu
DEV = "cuda"
ETAS = (0.0, 0.5, 1.0)
TAU_GAPS = [2, 3, 9, 17]                      # gaps, tau_0 > 0, tau_{S-1} < T - 1 = 19


def gen(seed):
    return torch.Generator().manual_seed(seed)


def close(got, ref):
    """the criterion; returns the margin used (error / allowance) for the printed figure"""
    err, allow = float((got.double().cpu() - ref.double()).abs().max()), 5e-5 * max(1.0, float(ref.abs().max()))
    return err <= allow, err / allow


def oracle_chain(p, x, yhat, noise, omabs, tau, eta, mc=1):
    """[S + 1, M, C] float64: y_T = z_0 + yhat, then chain positions S-1 .. 1 and the last step; rows r = trial * B + image."""
    cf = coef64(omabs, tau, eta)
    S = len(tau)
    xe, yh = ref_cpu.encoder_x(p, x).repeat(mc, 1), yhat.repeat(mc, 1)
    y = noise[0].double() + yh.double()
    seq = [y]
    for i in range(S):
        j = S - 1 - i
        eps = ref_cpu.trunk(p, xe, y.float(), torch.tensor([tau[j]]), yh).double()
        cy, cm, ce, cz = cf[j]
        y = cy * y + cm * yh.double() + ce * eps + (cz * noise[i + 1].double() if j >= 1 else 0.0)
        seq.append(y)
    return torch.stack(seq)


def engine_for(ps, dims, max_rows=None):
    from nested_diffusion_amd.engine import EnsembleEngine
    D, H, F, Cc, T, B = dims
    eng = EnsembleEngine(Cc, D, H, F, T, n_members=len(ps), max_batch=B, max_rows=max_rows or B)
    for k, p in enumerate(ps):
        eng.load_member(k, p)
    alphas, omabs = ref_cpu.schedule_tables("linear", T, 1e-4, 0.02)
    eng.set_schedule(alphas, omabs)
    return eng, omabs


def plan_of(omabs, tau, eta):
    from nested_diffusion_amd.diffusion_utils import sampler_plan
    return sampler_plan(omabs, tau, eta)


# ---- 1. whole trajectories ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,Cc", [(48, 1), (64, 3), (48, 8)])
def test_trajectories_over_a_sequence_with_gaps_and_the_shortest_chains(F, Cc):
    """T = 20: tau = [2, 3, 9, 17] (gaps, neither end of the schedule), S = 1 (tau = [5]: only the last step) and S = 2 (tau = [0, 19]),
    each at eta 0, 0.5 and 1; B = 5 images x mc = 2 trials (rows r = trial * B + image), two members in one launch."""
    D, H, T, B, mc = 64, 32, 20, 5, 2
    ps = [ref_cpu.init_cond_model_params(D, H, F, Cc, T, seed=3 + k) for k in range(2)]
    eng, omabs = engine_for(ps, (D, H, F, Cc, T, B), B * mc)
    g = gen(100 + F + Cc)
    x = torch.rand(B, D, generator=g)
    yhat = torch.softmax(torch.randn(2, B, Cc, generator=g), -1)
    eng.encode(x)
    for tau in (TAU_GAPS, [5], [0, 19]):
        S = len(tau)
        noise = torch.randn(2, S, B * mc, Cc, generator=g)
        for eta in ETAS:
            eng.set_sampler(plan_of(omabs, tau, eta))
            assert eng.sampler_steps() == S and eng.loop_form() == "graph_nodes"
            seq = eng.sample(yhat.cuda(), yhat.cuda(), noise.cuda(), mc=mc, return_seq=True)      # T defaults to the plan's S
            assert tuple(seq.shape) == (2, S + 1, B * mc, Cc)
            y0 = eng.sample(yhat.cuda(), yhat.cuda(), noise.cuda(), mc=mc, T=S)
            assert torch.equal(y0, seq[:, -1])
            for k in range(2):
                ref = oracle_chain(ps[k], x, yhat[k], noise[k], omabs, tau, eta, mc)
                assert torch.equal(seq[k, 0].cpu(), (noise[k, 0] + yhat[k].repeat(mc, 1)))          # y_T = z_0 + y_T_mean: exact
                ok, frac = close(seq[k], ref)
                print(f"F={F} C={Cc} tau={tau} eta={eta} member {k}: {frac:.3f} of the allowance")
                assert ok, (tau, eta, k, frac)


@pytest.mark.parametrize("skip_type", ["uniform", "quadratic"])
def test_trajectories_at_T_1000_with_a_contractive_member(skip_type):
    """The shipped schedule length with the denoiser-structured member (a random-weight member amplifies its start by ~160 over this
    schedule: nothing to compare), S = 20 of the 1000 timesteps, uniform and quadratic, eta 0 / 0.5 / 1: embedding rows up to 999, gaps of
    ~50 timesteps, and the quadratic sequence's consecutive timesteps at its low end."""
    from nested_diffusion_amd.diffusion_utils import timestep_sequence
    D, H, F, Cc, T, B = 64, 32, 64, 3, 1000, 5
    p = ref_cpu.init_cond_model_params(D, H, F, Cc, T, seed=3, denoiser=True)
    eng, omabs = engine_for([p], (D, H, F, Cc, T, B))
    tau = timestep_sequence(T, 20, skip_type)
    g = gen(7)
    x = torch.rand(B, D, generator=g)
    yhat = torch.softmax(torch.randn(1, B, Cc, generator=g), -1)
    noise = torch.randn(1, len(tau), B, Cc, generator=g)
    eng.encode(x)
    for eta in ETAS:
        eng.set_sampler(plan_of(omabs, tau, eta))
        seq = eng.sample(yhat.cuda(), yhat.cuda(), noise.cuda(), return_seq=True)[0]
        ref = oracle_chain(p, x, yhat[0], noise[0], omabs, tau, eta)
        assert float(ref[-1].abs().max()) < 10.0
        ok, frac = close(seq, ref)
        print(f"T=1000 S={len(tau)} {skip_type} eta={eta}: {frac:.3f} of the allowance")
        assert ok, (eta, frac)


# ---- 2. eager, graph, stale graphs, clearing -----------------------------------------------------------------------------------------------
def test_eager_equals_graph_and_a_new_plan_of_the_same_length_is_not_served_a_stale_graph():
    D, H, F, Cc, T, B, mc = 64, 32, 64, 3, 20, 5, 2
    ps = [ref_cpu.init_cond_model_params(D, H, F, Cc, T, seed=13 + k) for k in range(2)]
    eng, omabs = engine_for(ps, (D, H, F, Cc, T, B), B * mc)
    g = gen(21)
    x = torch.rand(B, D, generator=g)
    yhat = torch.softmax(torch.randn(2, B, Cc, generator=g), -1).cuda()
    noise_T, noise_S = torch.randn(2, T, B * mc, Cc, generator=g).cuda(), torch.randn(2, 4, B * mc, Cc, generator=g).cuda()
    eng.encode(x)
    run = lambda nz, graph: eng.sample(yhat, yhat, nz, mc=mc, return_seq=True, use_graph=graph)     # noqa: E731
    default = run(noise_T, False)
    assert torch.equal(run(noise_T, True), default)
    eng.set_sampler(plan_of(omabs, TAU_GAPS, 0.5))
    a_eager = run(noise_S, False)
    assert torch.equal(run(noise_S, True), a_eager) and torch.equal(run(noise_S, True), a_eager)   # build, then replay
    eng.set_sampler(plan_of(omabs, [1, 4, 10, 19], 1.0))                                           # the same S, same buffers, same shape
    b_graph = run(noise_S, True)
    b_eager = run(noise_S, False)
    assert torch.equal(b_graph, b_eager) and not torch.equal(b_graph, a_eager)
    eng.set_sampler(plan_of(omabs, TAU_GAPS, 0.5))                                                 # and back
    assert torch.equal(run(noise_S, True), a_eager)
    eng.clear_sampler()
    assert eng.sampler_steps() == 0
    assert torch.equal(run(noise_T, True), default) and torch.equal(run(noise_T, False), default)   # the default path's bits


# ---- 3. the many-rows head -------------------------------------------------------------------------------------------------------------------
def test_many_rows_head_returns_the_per_row_heads_bits_under_a_plan(monkeypatch):
    """M = 132 rows (B = 33, mc = 4; a ragged ninth 16-row tile), F = 64: k_step_head_rows' coefficient instantiation against
    k_step_head's (ND_HEAD_PER_ROW=1), every state of the trajectory, eta = 0.5 (all four coefficients live); and against the oracle."""
    D, H, F, Cc, T, B, mc = 64, 32, 64, 3, 20, 33, 4
    p = ref_cpu.init_cond_model_params(D, H, F, Cc, T, seed=31)
    eng, omabs = engine_for([p], (D, H, F, Cc, T, B), B * mc)
    plan = eng.step_plan(B * mc)
    assert plan["kernel"] == "k_cond_gemm" and plan["b9"]
    g = gen(5)
    x = torch.rand(B, D, generator=g)
    yhat = torch.softmax(torch.randn(1, B, Cc, generator=g), -1)
    noise = torch.randn(1, 4, B * mc, Cc, generator=g)
    eng.encode(x)
    eng.set_sampler(plan_of(omabs, TAU_GAPS, 0.5))
    monkeypatch.delenv("ND_HEAD_PER_ROW", raising=False)
    rows = eng.sample(yhat.cuda(), yhat.cuda(), noise.cuda(), mc=mc, use_graph=False, return_seq=True).cpu()
    monkeypatch.setenv("ND_HEAD_PER_ROW", "1")
    per_row = eng.sample(yhat.cuda(), yhat.cuda(), noise.cuda(), mc=mc, use_graph=False, return_seq=True).cpu()
    monkeypatch.delenv("ND_HEAD_PER_ROW")
    assert torch.isfinite(rows).all() and torch.equal(rows, per_row)
    ok, frac = close(rows[0], oracle_chain(p, x, yhat[0], noise[0], omabs, TAU_GAPS, 0.5, mc))
    assert ok, frac


# ---- 4. more members than descriptors travel by value ----------------------------------------------------------------------------------------
def test_nine_members_through_the_device_tables_and_a_range_of_three():
    D, H, F, Cc, T, B, K = 64, 32, 48, 3, 20, 6, 9
    ps = [ref_cpu.init_cond_model_params(D, H, F, Cc, T, seed=300 + k) for k in range(K)]
    eng, omabs = engine_for(ps, (D, H, F, Cc, T, B))
    g = gen(8)
    x = torch.rand(B, D, generator=g)
    yhat = torch.softmax(torch.randn(K, B, Cc, generator=g), -1)
    noise = torch.randn(K, 4, B, Cc, generator=g)
    eng.encode(x)
    eng.set_sampler(plan_of(omabs, TAU_GAPS, 0.5))
    y0 = eng.sample(yhat.cuda(), yhat.cuda(), noise.cuda()).cpu()
    assert torch.equal(eng.sample(yhat.cuda(), yhat.cuda(), noise.cuda(), use_graph=False).cpu(), y0)
    for k in range(K):
        ok, frac = close(y0[k], oracle_chain(ps[k], x, yhat[k], noise[k], omabs, TAU_GAPS, 0.5)[-1])
        assert ok, (k, frac)
    sub = eng.sample(yhat[2:5].cuda(), yhat[2:5].cuda(), noise[2:5].cuda(), member0=2, n_members=3).cpu()      # by value
    assert torch.equal(sub, y0[2:5])
    for k in (2, 3, 4):                                                                                          # each of them alone
        one = eng.sample(yhat[k:k + 1].cuda(), yhat[k:k + 1].cuda(), noise[k:k + 1].cuda(), member0=k, n_members=1).cpu()
        assert torch.equal(one[0], sub[k - 2])


# ---- 5 / 6. eta = 0 reads one draw; the identity plan ---------------------------------------------------------------------------------------
def test_eta_0_ignores_every_draw_but_the_first_and_the_identity_plan_is_the_default_chain():
    D, H, F, Cc, T, B = 64, 32, 64, 3, 20, 5
    p = ref_cpu.init_cond_model_params(D, H, F, Cc, T, seed=3)
    eng, omabs = engine_for([p], (D, H, F, Cc, T, B))
    g = gen(17)
    x = torch.rand(B, D, generator=g)
    yhat = torch.softmax(torch.randn(1, B, Cc, generator=g), -1).cuda()
    eng.encode(x)
    n1 = torch.randn(1, 4, B, Cc, generator=g)
    n2 = torch.randn(1, 4, B, Cc, generator=g) * 100.0
    n2[:, 0] = n1[:, 0]
    eng.set_sampler(plan_of(omabs, TAU_GAPS, 0.0))
    a, b = eng.sample(yhat, yhat, n1.cuda()), eng.sample(yhat, yhat, n2.cuda())
    assert torch.equal(a, b)
    eng.set_sampler(plan_of(omabs, TAU_GAPS, 1.0))
    assert not torch.equal(eng.sample(yhat, yhat, n1.cuda()), eng.sample(yhat, yhat, n2.cuda()))
    # S = T, eta = 1: the reference's posterior in coefficient form against the default path's own arithmetic
    noise = torch.randn(1, T, B, Cc, generator=g).cuda()
    eng.clear_sampler()
    default = eng.sample(yhat, yhat, noise, return_seq=True).cpu()
    eng.set_sampler(plan_of(omabs, list(range(T)), 1.0))
    ident = eng.sample(yhat, yhat, noise, return_seq=True).cpu()
    ok, frac = close(ident, default)
    print(f"identity plan vs the default path: {frac:.3f} of the allowance")
    assert ok, frac
    assert torch.equal(ident[:, 0], default[:, 0])


# ---- 7. nd_predict_batch / the runner --------------------------------------------------------------------------------------------------------
def _runner(sample_steps, eta, seed=1):
    from nested_diffusion_amd.mapping import Classifier, GuidingConditioner, VisionTransformer
    from nested_diffusion_amd.runner import Diffusion
    ns = argparse.Namespace
    embed, heads, depth, img, patch, K, B, T, mc, Cc = 128, 2, 5, 32, 16, 5, 4, 20, 2, 2
    D, H, F = 3 * img * img, 64, 64
    vp = ref_cpu.init_vit_params(embed=embed, depth=depth, patch=patch, img=img, seed=3)
    mlps = [ref_cpu.init_classifier_params((img // patch) ** 2 * embed, widths=(64, 32, 16), seed=20 + i) for i in range(K)]
    members = [ref_cpu.init_cond_model_params(D, H, F, Cc, T, True, seed=40 + i) for i in range(K)]
    cfg = ns(data=ns(dataset="ChestXRay", num_classes=Cc), model=ns(data_dim=D, hidden_dim=H, feature_dim=F, arch="linear"),
             diffusion=ns(timesteps=T, beta_schedule="linear", beta_start=1e-4, beta_end=0.02, aux_cls=ns(arch="sevit"),
                          trained_aux_cls_ckpt_path="", trained_diffusion_ckpt_path=[[]], include_guidance=True),
             testing=ns(batch_size=B))
    cond = GuidingConditioner(VisionTransformer(vp, heads, "cuda:0"), [Classifier(m, "cuda:0") for m in mlps])
    args = ns(seed=seed, mc_trials=mc, sample_steps=sample_steps, skip_type="uniform", sample_type="generalized", eta=eta)
    r = Diffusion(args, cfg, device="cuda:0", conditioner=cond, noise_estimator_states=members)
    r.load_noise_estimators(max_batch=B)
    return r, members, (K, B, T, mc, Cc, img)


def test_predict_batch_under_a_plan_equals_nd_sample_and_reproduces_from_its_seed():
    r, members, (K, B, T, mc, Cc, img) = _runner(5, 0.5)
    S = r.sample_steps
    assert S == 5 and r.engine.sampler_steps() == 5 and r.plan.timesteps.tolist() == [0, 5, 10, 14, 19]
    g = gen(9)
    x = torch.rand(B, 3, img, img, generator=g).cuda()
    noise = torch.randn(K, S, B * mc, Cc, generator=g).cuda()
    first = r.predict_batch(x, noise=noise)                          # the eager pass of a new shape
    again = r.predict_batch(x, noise=noise)                          # the recorded graph
    assert torch.equal(first["samples"], again["samples"]) and torch.equal(first["prob"], again["prob"])
    eng = r.engine
    eng.encode(x.flatten(1))
    y0 = eng.sample(first["yhat"], first["yhat"], noise, mc=mc, T=S)
    assert torch.equal(y0.reshape(K * mc, B, Cc), first["samples"])
    for k in (0, K - 1):                                             # and it is the strided chain: the oracle on the library's own yhat
        ok, frac = close(y0[k], oracle_chain(members[k], x.flatten(1).cpu(), first["yhat"][k].cpu(), noise[k].cpu(), r.one_minus_alphas_bar_sqrt.cpu(),
                                             r.plan.timesteps.tolist(), 0.5, mc)[-1])
        assert ok, (k, frac)
    with pytest.raises(Exception, match="sampler plan holds S=5 steps, the call asks T=20"):
        eng.predict_batch(r.cond_pred_model.handle(B, img), x, None, mc, T, r.temperature)
    # library-drawn noise: keyed on (seed, shape, batch counter) -- a second runner with the same seed draws the same
    a1, a2 = r.predict_batch(x)["samples"], r.predict_batch(x)["samples"]
    r2, _, _ = _runner(5, 0.5)
    b1, b2 = r2.predict_batch(x)["samples"], r2.predict_batch(x)["samples"]
    assert torch.equal(a1, b1) and torch.equal(a2, b2) and not torch.equal(a1, a2)
    assert r.draw_noise(B, 0, B).shape == (K, S, B * mc, Cc)


# ---- 8. stateful refusals --------------------------------------------------------------------------------------------------------------------
def test_a_call_with_another_T_and_a_bad_plan_are_refused_and_write_nothing():
    from nested_diffusion_amd import _lib
    D, H, F, Cc, T, B = 64, 32, 48, 3, 20, 4
    p = ref_cpu.init_cond_model_params(D, H, F, Cc, T, seed=3)
    eng, omabs = engine_for([p], (D, H, F, Cc, T, B))
    lib = eng.lib
    eng.encode(torch.rand(B, D, generator=gen(1)))
    plan = plan_of(omabs, TAU_GAPS, 0.5)
    eng.set_sampler(plan)
    yhat = torch.softmax(torch.randn(1, B, Cc, generator=gen(2)), -1).cuda()
    noise = torch.randn(1, T, B, Cc, generator=gen(3)).cuda()
    out = torch.full((1, B, Cc), 7.0, device=DEV)
    seq = torch.full((1, T + 1, B, Cc), 7.0, device=DEV)
    good = eng.sample(yhat, yhat, noise[:, :4].contiguous())
    for use_graph in (0, 1):
        for T_bad in (T, 3, 5):
            rc = lib.nd_sample(eng.h, 0, 1, yhat.data_ptr(), yhat.data_ptr(), noise.data_ptr(), out.data_ptr(), seq.data_ptr(), B, 1, T_bad, use_graph, None)
            assert (rc, lib.nd_last_error().decode()) == (-3, f"sampler plan holds S=4 steps, the call asks T={T_bad} (nd_set_sampler)")
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((seq == 7.0).all())
    # a refused nd_set_sampler leaves the plan that is set, and its results
    i32, f32 = C.c_int32, C.c_float
    bad_tau, coef = (i32 * 4)(2, 3, 3, 17), (f32 * 16)(*plan.coef.flatten().tolist())
    assert lib.nd_set_sampler(eng.h, bad_tau, coef, 4, None) == -1 and "strictly increasing" in lib.nd_last_error().decode()
    nan = (f32 * 16)(*([0.5] * 15 + [float("nan")]))
    assert lib.nd_set_sampler(eng.h, (i32 * 4)(*TAU_GAPS), nan, 4, None) == -1 and "coefficient [3][3] is not finite" in lib.nd_last_error().decode()
    assert lib.nd_set_sampler(eng.h, (i32 * 4)(*TAU_GAPS), coef, T + 1, None) == -1 and "S=21 outside [0,20]" in lib.nd_last_error().decode()
    assert eng.sampler_steps() == 4
    assert torch.equal(eng.sample(yhat, yhat, noise[:, :4].contiguous()), good)
    with pytest.raises(ValueError):
        eng.set_sampler((torch.tensor([1, 2]), torch.zeros(3, 4)))
    with pytest.raises(_lib.NdError, match="outside"):
        eng.set_sampler((torch.tensor([1, 20]), torch.zeros(2, 4)))
    # nd_eps_theta and nd_p_sample do not look at the plan
    eng.clear_sampler()
    y = torch.randn(B, Cc, generator=gen(4)).cuda()
    e0, s0 = eng.eps_theta(0, y, yhat[0], 7), eng.p_sample(0, y, yhat[0], yhat[0], 7, z=noise[0, 0])
    eng.set_sampler(plan)
    assert torch.equal(eng.eps_theta(0, y, yhat[0], 7), e0) and torch.equal(eng.p_sample(0, y, yhat[0], yhat[0], 7, z=noise[0, 0]), s0)


def test_p_sample_loop_takes_timesteps_and_returns_S_plus_1_states():
    from nested_diffusion_amd import diffusion_utils as du
    from nested_diffusion_amd.latent_model import ConditionalModel
    D, H, F, Cc, T, B = 64, 32, 48, 3, 20, 4
    p = ref_cpu.init_cond_model_params(D, H, F, Cc, T, seed=3)
    alphas, omabs = ref_cpu.schedule_tables("linear", T, 1e-4, 0.02)
    ns = types.SimpleNamespace
    cfg = ns(model=ns(data_dim=D, hidden_dim=H, feature_dim=F, arch="linear"), data=ns(num_classes=Cc, dataset="ChestXRay"), diffusion=ns(timesteps=T))
    model = ConditionalModel(cfg, guidance=True, max_batch=B)
    model.load_state_dict(p)
    model = model.to(DEV).eval()
    g = gen(6)
    x = torch.rand(B, D, generator=g)
    yhat = torch.softmax(torch.randn(B, Cc, generator=g), -1)
    noise = torch.randn(4, B, Cc, generator=g)
    seq = du.p_sample_loop(model, x.cuda(), yhat.cuda(), yhat.cuda(), T, alphas, omabs, noise=noise.cuda(), timesteps=TAU_GAPS, eta=0.5)
    assert len(seq) == 5
    ok, frac = close(torch.stack(seq), oracle_chain(p, x, yhat, noise, omabs, TAU_GAPS, 0.5))
    assert ok, frac
    assert model.hip_engine().sampler_steps() == 0               # the model's engine keeps no plan
    full = du.p_sample_loop(model, x.cuda(), yhat.cuda(), yhat.cuda(), T, alphas, omabs, only_last_sample=True,
                            noise=torch.randn(T, B, Cc, generator=g).cuda())
    assert tuple(full.shape) == (B, Cc)


# ---- 9. the input gradient through a strided chain --------------------------------------------------------------------------------------------
def strided_loop(pp, x, yh, noise, cf, tau, dtype):
    """the chain in `dtype` with autograd: coefficients cf (formed in double; rounded to fp32 first for the fp32 run, as the library does)"""
    S = len(tau)
    c = lambda v: torch.tensor(v, dtype=torch.float32).to(dtype) if dtype == torch.float32 else torch.tensor(v, dtype=dtype)   # noqa: E731
    xe = ref_cpu.encoder_x(pp, x)
    y = noise[0] + yh
    for i in range(S):
        j = S - 1 - i
        eps = ref_cpu.trunk(pp, xe, y, torch.tensor([tau[j]]), yh)
        cy, cm, ce, cz = (c(v) for v in cf[j])
        y = cy * y + cm * yh + ce * eps + (cz * noise[i + 1] if j >= 1 else 0.0)
    return y


def member_oracle(p, x_flat, yhat, noise, cot, cf, tau, mc, dtype):
    c = lambda t: t.to(dtype)                                  # noqa: E731
    x, yh = c(x_flat).clone().requires_grad_(True), c(yhat).clone().requires_grad_(True)
    pp = {k: c(v) for k, v in p.items() if v.is_floating_point()}
    y0 = strided_loop(pp, x.repeat(mc, 1), yh.repeat(mc, 1), c(noise), cf, tau, dtype)
    (y0 * c(cot)).sum().backward()
    return y0.detach(), x.grad, yh.grad


@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_sampler_tape_with_a_plan_forward_and_backward(eta):
    """One member, the shapes of test_gpu_ensemble_grad.py's smallest member test (D = 64, H = 32, F = 48, C = 2; B, mc in {1, 3}), T = 12
    timesteps of which tau = [1, 4, 5, 10] are walked.  Forward against EnsembleEngine.sample under the same plan: the criterion
    5e-5 * max(1, |ref|), NOT bit equality -- the tape evaluates eps through ops.linear (nd_linear's summation order), the engine through
    its step blocks, and the existing full-chain test claims a tolerance between them as well; the update itself is the same device
    function.  Backward against float64 autograd through the strided chain with that file's rule: e32 = the fp32 oracle's distance to
    float64 (<= 5e-6 asserted on the inputs), the GPU within max(1e-5, 4 e32) in relative L2."""
    from nested_diffusion_amd.ensemble_grad import SamplerTape
    from test_gpu_attack import rel_l2
    from test_gpu_ensemble_grad import E32_MAX, tol
    D, H, F, Cc, T = 64, 32, 48, 2, 12
    tau = [1, 4, 5, 10]
    p = ref_cpu.init_cond_model_params(D, H, F, Cc, T, seed=42)
    alphas, omabs = ref_cpu.schedule_tables("linear", T, 1e-4, 0.02)
    cf = coef64(omabs, tau, eta)
    tape = SamplerTape(p, alphas, omabs, DEV, timesteps=tau, eta=eta)
    assert tape.S == 4 and tape.T == T
    for B, mc in ((1, 1), (3, 3)):
        g = gen(7 * B + mc)
        x = torch.rand(B, D, generator=g)
        yhat = torch.softmax(torch.randn(B, Cc, generator=g), dim=1)
        noise, cot = torch.randn(4, B * mc, Cc, generator=g), torch.randn(B * mc, Cc, generator=g)
        ref = member_oracle(p, x, yhat, noise, cot, cf, tau, mc, torch.float64)
        r32 = member_oracle(p, x, yhat, noise, cot, cf, tau, mc, torch.float32)
        y0 = tape.forward(x.to(DEV), yhat.to(DEV), noise.to(DEV))
        assert len(tape._tape["steps"]) == 4                     # the tape holds S steps
        dx, dyhat = tape.backward(cot.to(DEV))
        for name, got, want, w32 in zip(("y0", "dx_flat", "dyhat"), (y0, dx, dyhat), ref, r32):
            e32, r = rel_l2(w32, want), rel_l2(got, want)
            print(f"eta={eta} B={B} mc={mc} {name}: e32 {e32:.3e} gpu {r:.3e}")
            assert e32 <= E32_MAX, (name, "the inputs are ill-conditioned", e32)
            assert r <= tol(e32), (name, B, mc, r, e32)
        eng, _ = engine_for([p], (D, H, F, Cc, T, B), B * mc)
        eng.encode(x)
        eng.set_sampler(plan_of(omabs, tau, eta))
        want = eng.sample(yhat[None].cuda(), yhat[None].cuda(), noise[None].cuda(), mc=mc)[0]
        ok, frac = close(y0, want.cpu())
        assert ok, (B, mc, frac)
        with pytest.raises(ValueError, match="noise must be"):
            tape.forward(x.to(DEV), yhat.to(DEV), torch.zeros(T, B * mc, Cc, device=DEV))


def test_ensemble_target_input_grad_through_a_strided_chain(record_property):
    """EnsembleTarget(sample_steps=4) at the shapes of test_gpu_ensemble_grad.py's whole-chain cases (K = 3, mc = 2, B = 3, 32 x 32 images,
    T = 12, denoiser-structured members): P, loss and dx against float64 autograd through conditioner -> softmax -> strided chains ->
    aggregation -> -log P[label], with that file's tolerance rule."""
    from nested_diffusion_amd.diffusion_utils import timestep_sequence
    from nested_diffusion_amd.ensemble_grad import EnsembleTarget
    from test_gpu_attack import rel_l2
    from test_gpu_cond_grad import build_model
    from test_gpu_ensemble_grad import B_IMG, D_IMG, E32_MAX, F_DIM, H_DIM, IMG, K, MC, TAU, config_of, tol
    T, S_ask, eta = 12, 4, 0.5
    cond, vp, mlps = build_model(2, IMG, (48, 32, 16))
    nets = [ref_cpu.init_cond_model_params(D_IMG, H_DIM, F_DIM, 2, T, seed=60 + k, denoiser=True) for k in range(K)]
    target = EnsembleTarget(cond, nets, config_of(T), mc=MC, temperature=TAU, seed=4, sample_steps=S_ask, skip_type="uniform", eta=eta)
    tau = timestep_sequence(T, S_ask, "uniform")
    assert target.steps == len(tau) == 4 and target.T == T and all(t.S == 4 for t in target.tapes)
    _, omabs = ref_cpu.schedule_tables("linear", T, 1e-4, 0.02)
    cf = coef64(omabs, tau, eta)
    x = torch.rand(B_IMG, 3, IMG, IMG, generator=gen(31))
    labels = torch.arange(B_IMG) % 2
    noise = torch.randn(K, 4, B_IMG * MC, 2, generator=gen(44))

    def oracle(dtype):
        c = lambda t: t.to(dtype)                                  # noqa: E731
        cp = lambda q: {k: c(v) for k, v in q.items() if v.is_floating_point()}     # noqa: E731
        xx = c(x).clone().requires_grad_(True)
        outs = ref_cpu.compute_guiding_prediction(cp(vp), [cp(m) for m in mlps], xx, 2, 3, full_vit=False)
        xf = xx.reshape(B_IMG, -1)
        samples = []
        for k in range(K):
            yh = torch.softmax(outs[k], dim=1)
            y0 = strided_loop(cp(nets[k]), xf.repeat(MC, 1), yh.repeat(MC, 1), c(noise[k]), cf, tau, dtype)
            samples += [y0[j * B_IMG:(j + 1) * B_IMG] for j in range(MC)]
        prob = ref_cpu.compute_ensemble_confidence(samples, TAU)
        loss = -torch.log(prob[torch.arange(B_IMG), labels])
        loss.sum().backward()
        return prob.detach(), xx.grad, loss.detach()

    ref, r32 = oracle(torch.float64), oracle(torch.float32)
    P, dx, loss = target.input_grad(x.to(DEV), labels.to(DEV), noise=noise.to(DEV))
    assert dx.shape == x.shape and bool(dx.isfinite().all())
    for name, got, want, w32 in zip(("P", "dx", "loss"), (P, dx, loss), ref, r32):
        e32, r = rel_l2(w32, want), rel_l2(got, want)
        print(f"strided chain {name}: e32 {e32:.3e} gpu {r:.3e}")
        record_property(f"strided_{name}", {"e32": e32, "gpu": r})
        assert e32 <= E32_MAX, (name, "the inputs are ill-conditioned", e32)
        assert r <= tol(e32), (name, r, e32)
    assert torch.equal(target.forward(x.to(DEV), noise=noise.to(DEV)), P)
    assert tuple(target.draw_noise(B_IMG).shape) == (K, 4, B_IMG * MC, 2)
    with pytest.raises(ValueError, match="noise must be"):
        target.input_grad(x.to(DEV), labels.to(DEV), noise=torch.zeros(K, T, B_IMG * MC, 2, device=DEV))
    with pytest.raises(ValueError, match="eta"):
        EnsembleTarget(cond, nets, config_of(T), mc=MC, temperature=TAU, sample_steps=4, eta=1.5)


# ---- 10. the CLI ----------------------------------------------------------------------------------------------------------------------------
def test_main_test_with_sample_steps_runs_S_steps_per_chain(tmp_path, capsys, monkeypatch):
    """`main --test --sample_steps 3 --eta 0.5` on checkpoints in the reference's layouts (test_gpu_cli's tiny run: 6 timesteps through
    --timesteps, which keeps its meaning): the run ends like any other -- the same report lines, config.yml and stdout.txt -- and the
    runner's engine held a plan of 3 steps; the same line without --sample_steps but with a --skip_type nobody knows runs the full chain."""
    import os
    from nested_diffusion_amd import main as nd_main
    from nested_diffusion_amd import mapping
    import nested_diffusion_amd.runner as runner_mod
    from test_gpu_cli import _write_run
    T, K, B = 6, 5, 4
    ypath, _, _, _, dims = _write_run(str(tmp_path), T=T, K=K, B=B)
    orig = mapping.load_conditioner
    monkeypatch.setattr(mapping, "load_conditioner", lambda path, ds, device="cuda", num_heads=12, dtype="f32": orig(path, ds, device, dims["heads"], dtype))
    monkeypatch.setattr(runner_mod, "load_conditioner", mapping.load_conditioner)
    seen = []
    test_atk = runner_mod.Diffusion.test_atk

    def spy(self, *a, **k):
        acc = test_atk(self, *a, **k)
        seen.append((self.sample_steps, self.engine.sampler_steps(), self.num_timesteps, tuple(self.last_probs.shape)))
        return acc
    monkeypatch.setattr(runner_mod.Diffusion, "test_atk", spy)
    base = ["--test", "--device", "0", "--loss", "card_onehot_conditional", "--config", ypath, "--exp", os.path.join(str(tmp_path), "results"),
            "--ni", "--preprocess", "grayscaled", "--timesteps", str(T), "--seed", "7", "--synthetic_batches", "2", "--mc_trials", "3"]
    assert nd_main.main(base + ["--doc", "strided", "--sample_steps", "3", "--eta", "0.5"]) == 0
    assert nd_main.main(base + ["--doc", "full", "--skip_type", "nobody_knows", "--eta", "9"]) == 0
    assert seen == [(3, 3, T, (2 * B, 2)), (T, 0, T, (2 * B, 2))]
    out = capsys.readouterr().out
    for key in ("Majority voting accuracy for MC:", "ECE:", "Average correct PIW per class:", "Average incorrect variances per class:"):
        assert out.count(key) == 2, out
    for doc in ("strided", "full"):
        log = os.path.join(str(tmp_path), "results", "logs", doc, "split_0")
        txt = open(os.path.join(log, "stdout.txt")).read()
        assert os.path.exists(os.path.join(log, "config.yml")) and "Testing procedure finished" in txt and "Traceback" not in txt, txt
        assert "throughput:" in txt
