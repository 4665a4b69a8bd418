"""Edge shapes and launch-plan coverage of the reverse-diffusion step (csrc/nd_step.hip, csrc/nd_sampler.hip, csrc/nd_cond_gemm.hip, the k_skinny
instantiations of csrc/nd_skinny_kernel.hpp), driven through EnsembleEngine and the C ABI with ref_cpu.init_cond_model_params members.

The plan `emit_loop` follows is restated here (`cond_gemm_plan`, `step_launch`) with the CU count as a parameter and cross-checked
against nd_step_plan / nd_skinny_plan for every shape used (tests/test_abi_and_host.py runs the same restatement at 256 CUs without a
device).  Each branch's shape is found by a small search at test time; a CU count that moves a branch out of the grid fails the search.

Branches and the tests that reach them (graph and eager forms of every loop, bit-equal):
- k_skinny: M <= 64 (`skinny_f32_nm1`), two 64-row passes (`skinny_f32_nm5`), fp16 at M > 128 with >= 3 passes (`skinny_f16_nm5`,
  `skinny_f16_nm1`); nm = 1 and 5; F % 64 != 0 in all four.  The step head writes fp32 h1 (frag16) or fp16 h1 (frag32h) per row.
- k_cond_gemm_b9: split = 1 (`b9_split1`) and the three cheapest distinct splits > 1 (`b9_split_a/b/c`), all with M % 16 != 0,
  M % 128 != 0 and F % 128 != 0; the many-rows head (k_step_head_rows, NT <= 64).
- per-row head writing a frag32b3 image and reducing more than 64 eps partials: F = 4224 (`b9_per_row_4224`, TN = 33) and F = 4160
  (`b9_per_row_4160`, ragged last column tile).
- k_cond_gemm (f32-input MFMA): F % 32 != 0 (`cond_f32_depth`), nm > 8 through the device tables (`cond_f32_nm9`, and the mixed
  member ranges test), ND_STEP_F32_MFMA=1 (`cond_f32_env`).
- C = 1..8 on both head forms (`test_head_every_class_count`).
- k_step_final in all four modes: the loop's y_0, nd_eps_theta, nd_p_sample at t >= 1 and at t = 0 (every case).
- mixed member ranges at M > 128 on one K = 11 handle, member_buffer following the last launch.
- workspace poisoning and shape shrinking.

References: the oracle's formulas (ref_cpu._cond_linear / _bn_eval, p_sample_given_eps, p_sample_t_1to0_given_eps) in float64 on the
GPU, from the same fp32 parameters.  Checks are stage-local: h1 from the kernel's own y_t, yhat and xe; h2 from its own h1; eps and y_0
from its own h2.  Each element's error is divided by its own magnitude: a block output u = A (W h) + C by |A| (|W| |h|) + |C| plus the
softplus value (softplus is 1-Lipschitz); eps by |W4| applied to the previous line's scale, plus |b4|.  Earlier steps: every seq[i+1]
against a float64 step from the kernel's seq[i], with the scales carried through the three blocks.  The posterior's fp32 coefficients
cancel near t = 1 in the reference's own arithmetic, so there the kernel must stay within 4x of torch's fp32 oracle against float64 plus
the per-element bar.  Caller-owned outputs are buffers of 0xFF bytes before each call."""
import ctypes as Cty
import functools

import pytest
import torch
import torch.nn.functional as Fn

from oracle import ref_cpu
from test_gpu_grad_edges import check, poisoned, stream

pytestmark = pytest.mark.gpu
DEV = "cuda"
GEMM_TOL = 1e-5                  # per-element normalised error of every stage (fp32 accumulation)
F16_ROUND = 2.0 ** -11           # one rounding of a stored fp16 activation (h1, h2 of an fp16 handle) ...
F16_SUBNORMAL = 2.0 ** -25       # ... and its absolute floor: half the spacing of fp16 subnormals (below 2^-14)
D_IN, H_IN = 64, 32              # encoder dims: the step does not depend on them
CG_CAND = (1, 2, 3, 4, 6, 8, 12, 16)


# ---- 1. the launch plan, restated ------------------------------------------------------------------------------------------------
def cond_gemm_plan(F, M, nm, half, ncu):
    """nd_cond_gemm_plan (csrc/nd_cond_gemm.hpp) for K = N = F."""
    use_tile = M > 128 and not half
    nfr, mfr, nch = -(-F // 16), -(-M // 16), F // 16
    TM, TN = -(-mfr // 8), -(-nfr // 8)
    tiles = nm * TM * TN
    plan = dict(use_tile=use_tile, TM=TM, TN=TN, tiles=tiles, ntl=2 * TN, n_full=tiles, rem=0, split=1)
    if not use_tile:
        return plan
    n_full = tiles // ncu * ncu
    rem, split = tiles - n_full, 1
    if rem > 0:
        t_tile = nch * 64.0 * 32.0 / 2000.0
        best = 1e30
        for s in CG_CAND:
            if s > 1 and (nch // s < 16 or rem * s > 512):
                continue
            rounds = ((rem * s + ncu - 1) // ncu) / s
            t = rounds * t_tile + (3.0 + rem * s * 65536.0 * 2.0 / 4.0e6 if s > 1 else 0.0)
            if t < best - 1e-9:
                best, split = t, s
    if split == 1:
        n_full, rem = tiles, 0
    plan.update(n_full=n_full, rem=rem, split=split)
    return plan


def pick_mt(M):
    """nd_pick_mt: 16-row fragments per k_skinny pass."""
    if M <= 16:
        return 1
    if M <= 32:
        return 2
    f = -(-M // 16)
    return 5 if (f + 4) // 5 < (f + 3) // 4 else 4


def step_launch(F, M, nm, half, ncu, f32_mfma=False):
    """the choices emit_loop makes for one launch over nm members at M rows (handle built for >= M rows)."""
    cg = cond_gemm_plan(F, M, nm, half, ncu)
    b9 = cg["use_tile"] and not half and F % 32 == 0 and not f32_mfma and nm <= 8
    NT = cond_gemm_plan(F, M, 1, half, ncu)["ntl"] if cg["use_tile"] else F // 16        # step_partials
    mt = pick_mt(M)
    return dict(cg, F=F, M=M, nm=nm, half=half, NT=NT, b9=b9,
                kernel="k_cond_gemm_b9" if b9 else "k_cond_gemm" if cg["use_tile"] else "k_skinny",
                head="k_step_head_rows" if b9 and NT <= 64 else "k_step_head",
                h1="frag32b3" if b9 else "frag32h" if half else "frag16",
                table="inline" if nm <= 8 else "device", mt=mt, passes=-(-M // (16 * mt)),
                wgs=cg["n_full"] + cg["rem"] * cg["split"])


def library_plan(F, M, nm, half):
    """what the library says (nd_step_plan, nd_skinny_plan, nd_skinny_row_fragments) at the current device's CU count."""
    from nested_diffusion_amd import _lib
    lib = _lib.load()
    out = (Cty.c_int * 8)()
    _lib.check(lib.nd_step_plan(F, M, nm, int(half), out), "nd_step_plan")
    got = dict(zip(("use_tile", "wgs", "n_full", "rem", "split", "NT", "TM", "TN"), list(out)))
    if not got["use_tile"]:
        o6 = (Cty.c_int * 6)()
        _lib.check(lib.nd_skinny_plan(F, F, M, nm, int(half), 1, o6), "nd_skinny_plan")
        got["passes"], got["mt"] = o6[1], lib.nd_skinny_row_fragments(M)
    return got


def assert_plan_matches_library(L):
    got = library_plan(L["F"], L["M"], L["nm"], L["half"])
    want = {k: (int(L[k]) if k != "use_tile" else int(bool(L[k]))) for k in got}
    if not L["use_tile"]:
        want["wgs"], want["n_full"] = got["wgs"], got["n_full"]          # the stream's geometry is reported separately
    assert got == want, (L, got)


def ragged_m(M):
    return M % 16 != 0 and M % 128 != 0


# every case: the search grid and the branch it must reach.  BM: (B, mc) pairs; Fs: feature dims; nms: members per launch
CASES = {
    "skinny_f32_nm1": dict(C=1, half=False, Fs=(80, 208, 1040), BM=[(B, 1) for B in (7, 23, 37, 61)], nms=(1,),
                           want=lambda L: L["kernel"] == "k_skinny" and L["M"] <= 64 and L["passes"] == 1 and L["F"] % 64),
    "skinny_f32_nm5": dict(C=3, half=False, Fs=(80, 208, 1040), BM=[(B, mc) for B in (13, 19, 23, 29, 33) for mc in (3, 4, 5)],
                           nms=(5,), want=lambda L: L["kernel"] == "k_skinny" and 64 < L["M"] <= 128 and L["passes"] == 2 and L["F"] % 64),
    "skinny_f16_nm5": dict(C=2, half=True, Fs=(96, 224, 1056), BM=[(B, mc) for B in (13, 23, 29) for mc in (7, 9, 11)], nms=(5,),
                           want=lambda L: L["kernel"] == "k_skinny" and L["M"] > 128 and L["passes"] >= 3 and L["F"] % 64),
    "skinny_f16_nm1": dict(C=7, half=True, Fs=(96, 224, 1056), BM=[(B, mc) for B in (13, 23, 29) for mc in (7, 9, 11)], nms=(1,),
                           want=lambda L: L["kernel"] == "k_skinny" and L["M"] > 128 and L["passes"] >= 3 and L["F"] % 64),
    "b9_split1": dict(C=4, half=False, Fs=(288, 544, 800), BM=[(B, mc) for B in (13, 23, 29) for mc in (7, 9, 11)], nms=(1, 2, 3),
                      want=lambda L: L["kernel"] == "k_cond_gemm_b9" and L["split"] == 1 and ragged_m(L["M"]) and L["F"] % 128
                      and L["head"] == "k_step_head_rows"),
    "b9_per_row_4224": dict(C=8, half=False, Fs=(4224,), BM=[(B, mc) for B in (13, 23, 29) for mc in (7, 9, 11)], nms=(1,),
                            want=lambda L: L["kernel"] == "k_cond_gemm_b9" and L["head"] == "k_step_head" and L["NT"] > 64
                            and ragged_m(L["M"])),
    "b9_per_row_4160": dict(C=5, half=False, Fs=(4160,), BM=[(B, mc) for B in (13, 23, 29) for mc in (7, 9, 11)], nms=(2,),
                            want=lambda L: L["kernel"] == "k_cond_gemm_b9" and L["head"] == "k_step_head" and L["NT"] > 64
                            and ragged_m(L["M"]) and L["F"] % 128),
    "cond_f32_depth": dict(C=2, half=False, Fs=(272, 528), BM=[(B, mc) for B in (13, 23, 29) for mc in (7, 9, 11)], nms=(1, 2),
                           want=lambda L: L["kernel"] == "k_cond_gemm" and L["F"] % 32 and ragged_m(L["M"])),
    "cond_f32_nm9": dict(C=3, half=False, Fs=(288, 544), BM=[(B, mc) for B in (13, 23, 29) for mc in (7, 9, 11)], nms=(9,),
                         want=lambda L: L["kernel"] == "k_cond_gemm" and L["table"] == "device" and ragged_m(L["M"])),
    "cond_f32_env": dict(C=6, half=False, Fs=(288, 544), BM=[(B, mc) for B in (13, 23, 29) for mc in (7, 9, 11)], nms=(2,),
                         f32_mfma=True, want=lambda L: L["kernel"] == "k_cond_gemm" and L["F"] % 32 == 0 and ragged_m(L["M"])),
}
SPLIT_CASE = dict(half=False, Fs=(544, 800, 1056, 1312, 1568, 2080), BM=[(B, mc) for B in (13, 23, 29) for mc in (7, 9, 11, 15)],
                  nms=tuple(range(1, 9)))
SPLIT_CLASSES = {"b9_split_a": 1, "b9_split_b": 2, "b9_split_c": 6}


def search(ncu, Fs, BM, nms, want, half=False, f32_mfma=False, **_):
    """the cheapest (F, B, mc, nm) of the grid whose restated launch satisfies `want` at `ncu` CUs."""
    for _, F, B, mc, nm in sorted((nm * F * F * B * mc, F, B, mc, nm) for F in Fs for B, mc in BM for nm in nms):
        L = step_launch(F, B * mc, nm, half, ncu, f32_mfma)
        if want(L):
            return dict(L, B=B, mc=mc)
    raise AssertionError(f"no shape of the grid reaches the branch on {ncu} CUs")


def split_shapes(ncu):
    """the three cheapest distinct k-splits > 1 of k_cond_gemm_b9 with ragged M and ragged F, one shape each."""
    found = {}
    for s in CG_CAND[1:]:
        try:
            found[s] = search(ncu, want=lambda L, s=s: L["kernel"] == "k_cond_gemm_b9" and L["split"] == s and L["rem"] > 0
                              and ragged_m(L["M"]) and L["F"] % 128 and L["head"] == "k_step_head_rows", **SPLIT_CASE)
        except AssertionError:
            pass
    picked = sorted(found.values(), key=lambda L: L["nm"] * L["F"] ** 2 * L["M"])[:3]
    assert len(picked) == 3, f"only the k-splits {sorted(found)} are reachable on {ncu} CUs"
    return {name: dict(L, C=SPLIT_CLASSES[name]) for name, L in zip(SPLIT_CLASSES, picked)}


def all_case_shapes(ncu):
    """every case of CASES and the three split cases, resolved at `ncu` CUs: name -> launch (+ B, mc, C, f32_mfma)."""
    out = {name: dict(search(ncu, **spec), C=spec["C"], f32_mfma=spec.get("f32_mfma", False)) for name, spec in CASES.items()}
    out.update({k: dict(v, f32_mfma=False) for k, v in split_shapes(ncu).items()})
    return out


def check_case_coverage(shapes):
    """the section-2 branches every run must reach, over the resolved case shapes."""
    Ls = list(shapes.values())
    sk = [L for L in Ls if L["kernel"] == "k_skinny"]
    assert any(L["M"] <= 64 for L in sk) and any(64 < L["M"] <= 128 and L["passes"] == 2 for L in sk)
    assert any(L["half"] and L["M"] > 128 and L["passes"] >= 3 for L in sk) and any(not L["half"] for L in sk)
    assert {1, 5} <= {L["nm"] for L in sk} and all(L["F"] % 64 for L in sk)
    b9 = [L for L in Ls if L["kernel"] == "k_cond_gemm_b9"]
    assert any(L["split"] == 1 for L in b9) and len({L["split"] for L in b9 if L["split"] > 1}) >= 3
    assert any(ragged_m(L["M"]) for L in b9) and any(L["F"] % 128 for L in b9)
    cg = [L for L in Ls if L["kernel"] == "k_cond_gemm"]
    assert any(L["F"] % 32 for L in cg) and any(L["table"] == "device" for L in cg) and any(L["f32_mfma"] for L in cg)
    assert any(L["head"] == "k_step_head_rows" for L in Ls)
    per_row_img = [L for L in Ls if L["head"] == "k_step_head" and L["h1"] == "frag32b3"]
    assert any(L["NT"] > 64 and L["F"] == 4224 for L in per_row_img) and any(L["F"] == 4160 for L in per_row_img)
    assert {"frag16", "frag32h"} <= {L["h1"] for L in Ls if L["head"] == "k_step_head"}


@functools.lru_cache(None)
def ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(None)
def device_shapes():
    return all_case_shapes(ncu())


def test_plan_restatement_matches_library_at_device_cu_count():
    """every case shape against nd_step_plan at this device's CU count, and the coverage of section 2 over them."""
    from nested_diffusion_amd import _lib
    _lib.load()
    torch.zeros(1, device=DEV)
    shapes = device_shapes()
    for L in shapes.values():
        assert_plan_matches_library(L)
    check_case_coverage(shapes)
    for F in (272, 1056, 4160, 4224):                  # a wider sweep of the restated tile plan
        for M in (1, 64, 65, 128, 129, 161, 207, 640, 1400):
            for nm in (1, 3, 5, 9, 11):
                assert_plan_matches_library(step_launch(F, M, nm, False, ncu()))


# ---- references ------------------------------------------------------------------------------------------------------------------
def params64(p, half):
    """a member's parameters in float64 on the GPU; an fp16 handle streams lin2 / lin3 as fp16 (ref_cpu.fp16_operands)."""
    P = {k: v.to(DEV, torch.float64) for k, v in p.items() if v.is_floating_point()}
    if half:
        for k in ("lin2.lin.weight", "lin3.lin.weight"):
            P[k] = p[k].half().to(DEV, torch.float64)
    return P


def block64(P, name, norm, h, hscale, t):
    """BN(g_t (W h + b)) of a ConditionalLinear in float64 (the oracle's formula) and its scale |A| (|W| hscale) + |C|, where
    A = s g_t and C = s g_t b + o are the folded gain and shift."""
    u = ref_cpu._bn_eval(ref_cpu._cond_linear(P, name, h, torch.tensor([t], device=DEV)), P, norm)
    s = P[norm + ".weight"] / torch.sqrt(P[norm + ".running_var"] + ref_cpu.BN_EPS)
    g = P[name + ".embed.weight"][t]
    A, Cc = s * g, s * g * P[name + ".lin.bias"] + (P[norm + ".bias"] - P[norm + ".running_mean"] * s)
    return u, (hscale @ P[name + ".lin.weight"].abs().T) * A.abs() + Cc.abs()


def trunk64(P, xe, y, yhat, t, h1=None, h2=None):
    """the three blocks and lin4 in float64 with per-element scales.  h1 / h2 given (the kernel's own): the next stage starts
    from them; else the scales are carried through (the bar of a whole step)."""
    v = torch.cat([y, yhat], -1).double()
    u1, s1 = block64(P, "lin1", "unetnorm1", v, v.abs(), t)
    sp1 = Fn.softplus(u1)
    out = {"h1": xe * sp1, "s_h1": xe.abs() * (s1 + sp1)}
    x2, sx2 = (h1.double(), h1.double().abs()) if h1 is not None else (out["h1"], out["s_h1"])
    u2, s2 = block64(P, "lin2", "unetnorm2", x2, sx2, t)
    sp2 = Fn.softplus(u2)
    out.update(h2=sp2, s_h2=s2 + sp2)
    x3, sx3 = (h2.double(), h2.double().abs()) if h2 is not None else (out["h2"], out["s_h2"])
    u3, s3 = block64(P, "lin3", "unetnorm3", x3, sx3, t)
    sp3 = Fn.softplus(u3)
    out["eps"] = sp3 @ P["lin4.weight"].T + P["lin4.bias"]
    out["s_eps"] = (s3 + sp3) @ P["lin4.weight"].abs().T + P["lin4.bias"].abs()
    return out


def posterior64(y, ym, eps, s_eps, z, t, alphas, omabs):
    """p_sample_given_eps (t >= 1, z given) or p_sample_t_1to0_given_eps (t = 0) in float64, its scale (eps carries s_eps), and
    the oracle's own fp32 value for the same inputs (the fp32-relative part of the bar)."""
    y, ym, eps = y.double(), ym.double(), eps.double()
    s = omabs.double()[t].item()
    sab = (1 - s * s) ** 0.5
    e32 = eps.float().cpu()
    if t == 0:
        ref = 1 / sab * (y - (1 - sab) * ym - eps * s)
        scale = (y.abs() + abs(1 - sab) * ym.abs() + (eps.abs() + s_eps) * s) / sab
        ref32 = ref_cpu.p_sample_t_1to0_given_eps(y.float().cpu(), ym.float().cpu(), e32, omabs)
        return ref, scale, ref32.to(DEV).double()
    a, s1 = alphas.double()[t].item(), omabs.double()[t - 1].item()
    sab1, sa = (1 - s1 * s1) ** 0.5, a ** 0.5
    g0, g1, g2 = (1 - a) * sab1 / (s * s), s1 * s1 * sa / (s * s), 1 + (sab - 1) * (sa + sab1) / (s * s)
    bh = s1 * s1 / (s * s) * (1 - a)
    zd = z.double()
    ref = g0 * (1 / sab * (y - (1 - sab) * ym - eps * s)) + g1 * y + g2 * ym + bh ** 0.5 * zd
    scale = (abs(g0) / sab * (y.abs() + abs(1 - sab) * ym.abs() + (eps.abs() + s_eps) * s) + abs(g1) * y.abs() + abs(g2) * ym.abs()
             + bh ** 0.5 * zd.abs())
    ref32 = ref_cpu.p_sample_given_eps(y.float().cpu(), ym.float().cpu(), e32, t, alphas, omabs, z.float().cpu())
    return ref, scale, ref32.to(DEV).double()


WORST = {}                        # (stage, kernel) -> worst normalised error seen in this module (printed at its end)
KERNEL = ["?"]                    # the step-block kernel of the case being checked


def assert_stage(got, ref, scale, what, tol=GEMM_TOL, rounding=0.0, fp32_ref=None):
    """|got - ref| <= tol * scale + rounding * |ref| (+ 4 |fp32_ref - ref|) per element; NaN fails.  rounding = F16_ROUND: the
    stored value is an fp16, whose subnormals are spaced 2^-24 apart."""
    got = got.double()
    slack = rounding * ref.abs() + (F16_SUBNORMAL if rounding == F16_ROUND else 0.0)
    if fp32_ref is not None:
        slack = slack + 4 * (fp32_ref - ref).abs()
    err = ((got - ref).abs() - slack).clamp_min(0) / scale.clamp_min(1e-300)
    bad = ~(err <= tol)
    if bool(bad.any()):
        idx = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements off the bar {tol:g}, first at {idx}: got "
                             f"{float(got[idx])}, want {float(ref[idx])}, scale {float(scale[idx])}; rows hit "
                             f"{bad.reshape(bad.shape[0], -1).any(1).nonzero().flatten()[:8].tolist()}")
    key = (what.split(":")[0], KERNEL[0])
    WORST[key] = max(WORST.get(key, 0.0), float(err.max()))


# ---- the engine and the C ABI ----------------------------------------------------------------------------------------------------
def members_for(F, C, T, K, seed, regime="randn"):
    ps = [ref_cpu.init_cond_model_params(D_IN, H_IN, F, C, T, True, seed=seed + k) for k in range(K)]
    if regime == "negative":                       # strongly negative pre-activations in all three blocks
        for p in ps:
            for name in ("lin1", "lin2", "lin3"):
                p[name + ".lin.bias"] = p[name + ".lin.bias"] - 30.0
    return ps


def make_engine(F, C, T, K, B, max_rows, half, members, fill=None):
    """EnsembleEngine with the members loaded; fill: 0xFF / 0 written over the whole workspace and re-bound first."""
    from nested_diffusion_amd.engine import EnsembleEngine
    eng = EnsembleEngine(C, D_IN, H_IN, F, T, n_members=K, max_batch=B, max_rows=max_rows, dtype="f16" if half else "f32")
    if fill is not None:
        eng.workspace.fill_(fill)
        base = (eng.workspace.data_ptr() + 255) & ~255
        check(eng.lib.nd_bind_workspace(eng.h, base, eng.lib.nd_workspace_bytes(Cty.byref(eng.cfg))), "nd_bind_workspace")
    for k, p in enumerate(members):
        eng.load_member(k, p)
    alphas, omabs = ref_cpu.schedule_tables("linear", T, 1e-4, 0.02)
    eng.set_schedule(alphas, omabs)
    eng.tables = (alphas, omabs)
    return eng


def inputs(K, B, M, C, T, D, seed, regime="randn"):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, D, generator=g)
    yhat = torch.softmax(torch.randn(K, B, C, generator=g), -1)
    ymean = torch.softmax(torch.randn(K, B, C, generator=g), -1)
    noise = torch.randn(K, T, M, C, generator=g)
    y = torch.randn(M, C, generator=g)
    z = torch.randn(M, C, generator=g)
    if regime == "big":                            # activations beyond softplus's threshold of 20 (as eps_big of the sampler tests)
        x, noise, y = x * 40.0, noise * 30.0, y * 30.0
    return {k: v.to(DEV) for k, v in dict(x=x, yhat=yhat, ymean=ymean, noise=noise, y=y, z=z).items()}


def sample_abi(eng, io, m0, nm, B, mc, T, use_graph, draw=False):
    """nd_sample into 0xFF outputs: (y0 [nm, M, C], seq [nm, T+1, M, C])."""
    M, C = B * mc, eng.C
    y0, seq = poisoned(nm, M, C), poisoned(nm, T + 1, M, C)
    yh, ym = io["yhat"][m0:m0 + nm].contiguous(), io["ymean"][m0:m0 + nm].contiguous()
    nz = None if draw else io["noise"][m0:m0 + nm].contiguous()
    check(eng.lib.nd_sample(eng.h, m0, nm, yh.data_ptr(), ym.data_ptr(), None if nz is None else nz.data_ptr(), y0.data_ptr(),
                            seq.data_ptr(), B, mc, T, int(use_graph), stream()), "nd_sample")
    torch.cuda.synchronize()
    assert torch.isfinite(y0).all() and torch.isfinite(seq).all(), "an output element was not written"
    assert torch.equal(seq[:, T], y0)
    return y0, seq


def eps_theta_abi(eng, k, y, yhat, t, B, mc):
    out = poisoned(B * mc, eng.C)
    check(eng.lib.nd_eps_theta(eng.h, k, y.data_ptr(), yhat.data_ptr(), t, out.data_ptr(), B, mc, stream()), "nd_eps_theta")
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    return out


def p_sample_abi(eng, k, y, yhat, ymean, z, t, B, mc):
    out = poisoned(B * mc, eng.C)
    check(eng.lib.nd_p_sample(eng.h, k, y.data_ptr(), yhat.data_ptr(), ymean.data_ptr(), z.data_ptr() if t > 0 else None, t,
                              out.data_ptr(), B, mc, stream()), "nd_p_sample")
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    return out


def rows_of(t, B, M):
    return t[torch.arange(M, device=t.device) % B]


def check_head_and_blocks(eng, k, P, y, yhat_rows, t, B, M, what):
    """stage-local: h1 (member_buffer 1) from (y, yhat, xe), h2 from the kernel's h1; returns the float64 eps from the kernel's h2."""
    half = eng.dtype == 1
    xe = rows_of(eng.member_buffer(k, 0, B).double(), B, M)
    h1, h2 = eng.member_buffer(k, 1, M), eng.member_buffer(k, 2, M)
    torch.cuda.synchronize()
    r = trunk64(P, xe, y, yhat_rows, t)
    assert_stage(h1, r["h1"], r["s_h1"], f"h1: {what}", rounding=F16_ROUND if half else 0.0)
    r = trunk64(P, xe, y, yhat_rows, t, h1=h1)
    assert_stage(h2, r["h2"], r["s_h2"], f"h2: {what}", rounding=F16_ROUND if half else 0.0)
    return trunk64(P, xe, y, yhat_rows, t, h1=h1, h2=h2)


def check_loop(eng, Ps, io, m0, nm, B, mc, T, seq, what):
    """seq[i+1] from a float64 step on the kernel's seq[i]; at t = 0 h1, h2 and y_0 stage by stage (member_buffer)."""
    M = B * mc
    alphas, omabs = eng.tables
    # an fp16 handle rounds h1 and h2 to fp16 once each: carried through a whole step, two such roundings of the scale
    tol = GEMM_TOL + 2 * F16_ROUND if eng.dtype == 1 else GEMM_TOL
    for g in range(nm):
        k = m0 + g
        P = Ps[k]
        yh, ym = rows_of(io["yhat"][k], B, M).double(), rows_of(io["ymean"][k], B, M).double()
        assert torch.equal(seq[g, 0], io["noise"][k, 0] + rows_of(io["ymean"][k], B, M))      # y_T = noise[0] + y_T_mean, exact
        xe = rows_of(eng.member_buffer(k, 0, B).double(), B, M)
        for i in range(T - 1):
            t = T - 1 - i
            r = trunk64(P, xe, seq[g, i].double(), yh, t)
            ref, scale, ref32 = posterior64(seq[g, i], ym, r["eps"], r["s_eps"], io["noise"][k, i + 1], t, alphas, omabs)
            assert_stage(seq[g, i + 1], ref, scale, f"step: {what} member {k} step {i} (t={t})", tol=tol,
                         fp32_ref=ref32)
        r = check_head_and_blocks(eng, k, P, seq[g, T - 1].double(), yh, 0, B, M, f"{what} member {k} (loop, t=0)")
        ref, scale, ref32 = posterior64(seq[g, T - 1], ym, r["eps"], r["s_eps"], None, 0, alphas, omabs)
        assert_stage(seq[g, T], ref, scale, f"y0: {what} member {k}", fp32_ref=ref32)


def check_single_evals(eng, Ps, io, k, B, mc, T, what):
    """k_step_final modes 1 (eps_theta), 2 (p_sample t >= 1) and 3 (p_sample t = 0), each stage-local."""
    M = B * mc
    alphas, omabs = eng.tables
    yh, ym = io["yhat"][k].contiguous(), io["ymean"][k].contiguous()
    yhr, ymr = rows_of(yh, B, M).double(), rows_of(ym, B, M).double()
    for t in sorted({0, 1, T - 1}):
        eps = eps_theta_abi(eng, k, io["y"], yh, t, B, mc)
        r = check_head_and_blocks(eng, k, Ps[k], io["y"].double(), yhr, t, B, M, f"{what} eps_theta t={t}")
        assert_stage(eps, r["eps"], r["s_eps"], f"eps: {what} eps_theta t={t}")
        out = p_sample_abi(eng, k, io["y"], yh, ym, io["z"], t, B, mc)
        r = check_head_and_blocks(eng, k, Ps[k], io["y"].double(), yhr, t, B, M, f"{what} p_sample t={t}")
        ref, scale, ref32 = posterior64(io["y"], ymr, r["eps"], r["s_eps"], io["z"], t, alphas, omabs)
        assert_stage(out, ref, scale, f"{'y0' if t == 0 else 'p_sample'}: {what} p_sample t={t}", fp32_ref=ref32)


def run_case(L, seed, monkeypatch, regime="randn", T=4):
    F, B, mc, nm, C, half = L["F"], L["B"], L["mc"], L["nm"], L["C"], L["half"]
    M = B * mc
    KERNEL[0] = L["kernel"] + ("/fp16" if half else "")
    if L.get("f32_mfma"):
        monkeypatch.setenv("ND_STEP_F32_MFMA", "1")
    else:
        monkeypatch.delenv("ND_STEP_F32_MFMA", raising=False)
    members = members_for(F, C, T, nm, seed, regime)
    eng = make_engine(F, C, T, nm, B, M, half, members)
    plan = eng.step_plan(M, nm)
    assert plan["kernel"] == ("k_skinny" if L["kernel"] == "k_skinny" else "k_cond_gemm") and plan["b9"] == L["b9"], (plan, L)
    assert_plan_matches_library(L)
    io = inputs(nm, B, M, C, T, D_IN, seed + 100, regime)
    eng.encode(io["x"])
    y0_g, seq_g = sample_abi(eng, io, 0, nm, B, mc, T, True)
    y0_e, seq_e = sample_abi(eng, io, 0, nm, B, mc, T, False)
    assert torch.equal(seq_g, seq_e), "graph and eager forms differ"
    Ps = [params64(p, half) for p in members]
    check_loop(eng, Ps, io, 0, nm, B, mc, T, seq_e, f"{L['kernel']} F={F} M={M} nm={nm} C={C}")
    check_single_evals(eng, Ps, io, nm - 1, B, mc, T, f"F={F} M={M} C={C}")
    return eng, io, members


# ---- 2. branches ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES) + list(SPLIT_CLASSES))
def test_step_branch(case, monkeypatch, record_property):
    L = device_shapes()[case]
    record_property("shape", {k: L[k] for k in ("F", "B", "mc", "M", "nm", "C", "kernel", "head", "h1", "split", "NT", "passes")})
    run_case(L, 1000 + 17 * list(device_shapes()).index(case), monkeypatch)


@pytest.mark.parametrize("C", range(1, 9))
def test_head_every_class_count(C, monkeypatch):
    """C = 1..8 on both head forms: k_step_head_rows (b9, M = 145) and k_step_head writing fp32 h1 (k_skinny, M = 29)."""
    F, B = 288, 29
    rows = dict(step_launch(F, B * 5, 1, False, ncu()), B=B, mc=5, C=C)
    per_row = dict(step_launch(F, B, 1, False, ncu()), B=B, mc=1, C=C)
    assert rows["head"] == "k_step_head_rows" and per_row["head"] == "k_step_head" and per_row["h1"] == "frag16"
    run_case(rows, 40 + C, monkeypatch)
    run_case(per_row, 60 + C, monkeypatch)


@pytest.mark.parametrize("regime", ["big", "negative"])
@pytest.mark.parametrize("case", ["skinny_f32_nm1", "b9_split_a", "b9_per_row_4160"])
def test_step_ill_conditioned_inputs(case, regime, monkeypatch):
    """activations beyond softplus's threshold of 20 and strongly negative pre-activations (lin biases - 30), same bars."""
    run_case(device_shapes()[case], 2000 + len(regime), monkeypatch, regime=regime)


def test_mixed_member_ranges_on_one_handle(monkeypatch):
    """K = 11 at M > 128: all 11 (device tables, f32 k_cond_gemm into h1 / h2), members 0-2 (inline, b9 images), all 11 again.
    Each result is bit-equal to a fresh engine's; member_buffer returns the layout the last launch over a member wrote."""
    monkeypatch.delenv("ND_STEP_F32_MFMA", raising=False)
    F, C, T, K, B, mc = 288, 3, 3, 11, 23, 7
    M = B * mc
    assert step_launch(F, M, K, False, ncu())["kernel"] == "k_cond_gemm" and step_launch(F, M, 3, False, ncu())["b9"]
    members = members_for(F, C, T, K, 700)
    Ps = [params64(p, False) for p in members]
    io = inputs(K, B, M, C, T, D_IN, 701)
    eng = make_engine(F, C, T, K, B, M, False, members)
    eng.encode(io["x"])
    KERNEL[0] = "mixed K=11"

    def fresh(m0, nm):
        e = make_engine(F, C, T, K, B, M, False, members)
        e.encode(io["x"])
        return sample_abi(e, io, m0, nm, B, mc, T, True)[1]

    for m0, nm in ((0, K), (0, 3), (0, K)):
        for graph in (True, False):
            seq = sample_abi(eng, io, m0, nm, B, mc, T, graph)[1]
            assert torch.equal(seq, fresh(m0, nm)), (m0, nm, graph)
        check_loop(eng, Ps, io, m0, nm, B, mc, T, seq, f"mixed [{m0},{m0 + nm})")
        if nm == 3:                       # members 3.. still hold what the 11-member launch wrote
            h1_kept = eng.member_buffer(5, 1, M)
            assert torch.equal(h1_kept, h1_after_all)
        else:
            h1_after_all = eng.member_buffer(5, 1, M)


POISON_CASES = ["skinny_f32_nm5", "b9_split_b", "cond_f32_nm9"]


@pytest.mark.parametrize("case", POISON_CASES)
def test_poisoned_workspace_changes_no_bit(case, monkeypatch):
    """the whole EnsembleEngine.workspace as 0xFF bytes (fp32 / bf16 / fp16 NaNs), re-bound (the library zeroes what it zeroes), then
    load_member -> set_schedule -> encode -> sample (graph, eager, in-library draws) -> eps_theta -> p_sample: bit-equal to an
    engine whose workspace started as zeros."""
    L = device_shapes()[case]
    monkeypatch.delenv("ND_STEP_F32_MFMA", raising=False)
    F, B, mc, nm, C, T = L["F"], L["B"], L["mc"], L["nm"], L["C"], 4
    M = B * mc
    members = members_for(F, C, T, nm, 800)
    io = inputs(nm, B, M, C, T, D_IN, 801)
    results = []
    for fill in (0, 0xFF):
        eng = make_engine(F, C, T, nm, B, M, False, members, fill=fill)
        eng.encode(io["x"])
        eng.seed(5)
        r = [sample_abi(eng, io, 0, nm, B, mc, T, g) for g in (True, False)]
        r.append(sample_abi(eng, io, 0, nm, B, mc, T, True, draw=True))
        yh, ym = io["yhat"][0].contiguous(), io["ymean"][0].contiguous()
        r.append(eps_theta_abi(eng, 0, io["y"], yh, T - 1, B, mc))
        r += [p_sample_abi(eng, 0, io["y"], yh, ym, io["z"], t, B, mc) for t in (T - 1, 0)]
        results.append(r)
        del eng
    for a, b in zip(*results):
        a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
        for x, y in zip(a, b):
            assert torch.equal(x, y)


@pytest.mark.parametrize("mcs", [(9, 7), (9, 3), (15, 11)])
def test_shrinking_rows_reads_no_stale_rows(mcs, monkeypatch):
    """a large ragged M, then a smaller ragged M on the same handle: bit-equal to a fresh handle that only ran the smaller M
    (stale pad rows of h1 / h2, the images, epart or tile_ws must not be read).  (9, 3) crosses from the tiled blocks to k_skinny."""
    monkeypatch.delenv("ND_STEP_F32_MFMA", raising=False)
    F, C, T, nm, B = 1056, 2, 3, 2, 23
    big, small = mcs
    members = members_for(F, C, T, nm, 900)
    io = inputs(nm, B, B * big, C, T, D_IN, 901)
    io_small = dict(io, noise=io["noise"][:, :, : B * small].contiguous(), y=io["y"][: B * small].contiguous(),
                    z=io["z"][: B * small].contiguous())
    outs = []
    for warm in (True, False):
        eng = make_engine(F, C, T, nm, B, B * big, False, members)
        eng.encode(io["x"])
        if warm:
            sample_abi(eng, io, 0, nm, B, big, T, True)
            eps_theta_abi(eng, 1, io["y"], io["yhat"][1].contiguous(), 1, B, big)
        o = [sample_abi(eng, io_small, 0, nm, B, small, T, g)[1] for g in (True, False)]
        o.append(eps_theta_abi(eng, 1, io_small["y"], io["yhat"][1].contiguous(), 1, B, small))
        outs.append(o)
        del eng
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.fixture(scope="module", autouse=True)
def report_worst_normalised_errors():
    """prints the worst per-element normalised error of each stage over the module (the bars are asserted per check)."""
    yield
    for (stage, kernel), err in sorted(WORST.items()):
        print(f"\nworst normalised error {stage:8s} {kernel:22s} {err:.3e}", end="")
