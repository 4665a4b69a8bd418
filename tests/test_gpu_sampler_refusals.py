"""The row refusals of the entry points that run the reverse loop (csrc/nd_sampler.hip: nd_sample, nd_predict_batch, nd_p_sample,
nd_eps_theta), pinned word for word: the return code and the whole nd_last_error text, one input per fault.  Every call here is
refused before anything is launched; the order of the checks is B, then mc and B*mc, then T, then the schedule (then, where the
entry point relies on an earlier nd_encode, its B).  nd_eps_theta has its own, shorter texts and no schedule check."""
import ctypes as C

import pytest
import torch

from oracle import ref_cpu

pytestmark = pytest.mark.gpu

ARG, STATE = -1, -3
K, D, H, F, Cc, N_STEPS, MAX_B, MAX_ROWS, SCHED = 2, 48, 64, 64, 2, 10, 4, 12, 6
B0, MC0, T0 = 4, 3, 6                       # the good call every case departs from in one argument

ROWS = {                                     # nd_sample / nd_predict_batch / nd_p_sample (check_rows)
    "B=0": (dict(B=0), ARG, "B=0 outside [1,4]"),
    "B=5": (dict(B=5), ARG, "B=5 outside [1,4]"),
    "mc=0": (dict(mc=0), ARG, "mc=0 outside [1,65535] or B*mc=0 exceeds max_rows=12"),
    "B*mc=16": (dict(mc=4), ARG, "mc=4 outside [1,65535] or B*mc=16 exceeds max_rows=12"),
    "T=0": (dict(T=0), ARG, "T=0 outside [1,10]"),
    "T=11": (dict(T=11), ARG, "T=11 outside [1,10]"),
    "T=7": (dict(T=7), STATE, "schedule holds 6 steps, need 7 (nd_set_schedule)"),
}
NULL = (dict(null=True), ARG, "NULL tensor")
SAMPLE = dict(ROWS, **{"encoded B": (dict(B=3), STATE, "nd_encode ran with B=4, sampling asks B=3"), "NULL": NULL,
                       "members": (dict(m0=1, nm=2), ARG, "member range [1,3) invalid")})
BATCH = dict(ROWS, NULL=NULL)
# the per-member entry points take t = T - 1; nd_p_sample refuses t < 0 before it looks at the rows
P_SAMPLE = dict(ROWS, **{"T=0": (dict(T=0), ARG, "t must be >= 0"), "NULL": NULL, "members": (dict(m0=2), ARG, "member range [2,3) invalid")})
EPS = {k: (a, ARG, "B/mc out of range") for k, (a, _, _) in ROWS.items() if k[0] != "T"}
EPS.update({"T=0": (dict(T=0), ARG, "t=-1 outside [0,10)"), "T=11": (dict(T=11), ARG, "t=10 outside [0,10)"), "NULL": NULL,
            "members": (dict(m0=2), ARG, "member range [2,3) invalid")})


@pytest.fixture(scope="module")
def rig():
    from nested_diffusion_amd import _lib
    from nested_diffusion_amd.engine import EnsembleEngine
    lib = _lib.load()
    eng = EnsembleEngine(Cc, D, H, F, N_STEPS, n_members=K, max_batch=MAX_B, max_rows=MAX_ROWS)
    for k in range(K):
        eng.load_member(k, ref_cpu.init_cond_model_params(D, H, F, Cc, N_STEPS, True, seed=70 + k))
    alphas, omabs = ref_cpu.schedule_tables("linear", SCHED, 1e-4, 0.02)
    eng.set_schedule(alphas, omabs)
    eng.encode(torch.rand(B0, D, generator=torch.Generator().manual_seed(1)))
    # a conditioner that fits the ensemble (3 x 4 x 4 = data_dim, one mapping MLP per member); created only: every call below is
    # refused before the conditioner is asked for anything
    cfg = _lib.NdCondConfig()
    cfg.img_size, cfg.patch, cfg.in_chans, cfg.embed_dim, cfg.num_heads, cfg.mlp_hidden, cfg.n_blocks, cfg.n_mlps = 4, 4, 3, 64, 1, 64, K, K
    for i in range(3):
        cfg.mlp_widths[i] = 16
    cfg.num_classes, cfg.max_batch, cfg.max_tokens, cfg.operand_dtype, cfg.ln_eps = Cc, 2 * MAX_B, 2, 0, 1e-6
    cond = C.c_void_p()
    _lib.check(lib.nd_cond_create(C.byref(cfg), C.byref(cond)), "nd_cond_create")
    buf = torch.zeros(4096, device="cuda")       # stands for every tensor argument: never read, never written
    torch.cuda.synchronize()
    yield lib, eng, cond, buf
    torch.cuda.synchronize()
    lib.nd_cond_destroy(cond)


def _refused(lib, rc, want_rc, want_text):
    assert (rc, lib.nd_last_error().decode()) == (want_rc, want_text)


def _args(case):
    a = dict(B=B0, mc=MC0, T=T0, null=False, m0=0, nm=K)
    a.update(case)
    return a


@pytest.mark.parametrize("name", sorted(SAMPLE))
@pytest.mark.parametrize("use_graph", [0, 1])
def test_nd_sample_refusals(rig, name, use_graph):
    lib, eng, _, buf = rig
    case, rc, text = SAMPLE[name]
    a, p = _args(case), buf.data_ptr()
    _refused(lib, lib.nd_sample(eng.h, a["m0"], a["nm"], None if a["null"] else p, p, p, p, None, a["B"], a["mc"], a["T"], use_graph, None), rc, text)


@pytest.mark.parametrize("name", sorted(BATCH))
@pytest.mark.parametrize("use_graph", [0, 1])
def test_nd_predict_batch_refusals(rig, name, use_graph):
    from nested_diffusion_amd import _lib
    lib, eng, cond, buf = rig
    case, rc, text = BATCH[name]
    a, p = _args(case), buf.data_ptr()
    out = _lib.NdBatchOut(p, p, p, p, p)
    _refused(lib, lib.nd_predict_batch(eng.h, cond, None if a["null"] else p, p, C.byref(out), a["B"], a["mc"], a["T"], 1.0, use_graph, None), rc, text)


@pytest.mark.parametrize("name", sorted(P_SAMPLE))
def test_nd_p_sample_refusals(rig, name):
    lib, eng, _, buf = rig
    case, rc, text = P_SAMPLE[name]
    a, p = _args(dict(case, m0=case.get("m0", 1))), buf.data_ptr()
    _refused(lib, lib.nd_p_sample(eng.h, a["m0"], None if a["null"] else p, p, p, p, a["T"] - 1, p, a["B"], a["mc"], None), rc, text)


@pytest.mark.parametrize("name", sorted(EPS))
def test_nd_eps_theta_refusals(rig, name):
    lib, eng, _, buf = rig
    case, rc, text = EPS[name]
    a, p = _args(dict(case, m0=case.get("m0", 1))), buf.data_ptr()
    _refused(lib, lib.nd_eps_theta(eng.h, a["m0"], None if a["null"] else p, p, a["T"] - 1, p, a["B"], a["mc"], None), rc, text)


def test_the_call_every_case_departs_from_is_accepted(rig):
    """So each case above holds one fault only (y_T_mean = yhat, library noise)."""
    lib, eng, _, _ = rig
    yhat = torch.softmax(torch.randn(K, B0, Cc, generator=torch.Generator().manual_seed(2)), -1).cuda()
    y0 = eng.sample(yhat, yhat, None, mc=MC0, T=T0)
    assert y0.shape[0] == K and bool(torch.isfinite(y0).all())
