"""Edge shapes and launch-plan coverage of the weight-streaming Linear (k_skinny MODE 0 / MODE 2 of csrc/nd_skinny_kernel.hpp, k_splitk_epilogue
of csrc/nd_skinny_m2.hip, linear_packed of csrc/nd_linear.hip, nd_pack_rows of csrc/nd_pack.hip), of the encoder hoist (nd_encode of csrc/nd_sampler.hip, with the
k_fold_bn folds of nd_load_member) and of the mapping MLP that runs on the same stream (Classifier, GuidingConditioner).

The launch plan is restated here (`skinny_plan` from nd_skinny_launch_impl, `linear_route` from nd_use_splitk / nd_cond_gemm_plan) with
the CU count as a parameter and cross-checked against nd_skinny_plan / nd_skinny_row_fragments / nd_linear_workspace_bytes for every shape
used (tests/test_abi_and_host.py runs the same restatement and the same coverage check at 256 CUs without a device).  Each branch's shape
is found by a small search at test time under a byte cap (weights + workspace <= 256 MB); a CU count that moves a branch out of the grid
fails the search.

Branches and the cases of LINEAR_CASES that reach them (`test_linear_branch`, both operand types):
- row fragments MT = 1, 2, 4, 5: `rows1` .. `rows128` (M = 1, 16, 17, 32, 33, 64, 65, 80, 81, 128); the clamped xp[mt] of a last row group
  whose trailing fragments lie beyond mtiles: `rows33`, `rows81`.
- NF = 1..6 with a workgroup of NF and one of NF - 1 fragments (nfr % wpm != 0): `nf1` .. `nf6` (MODE 0), `splitk_partial` (MODE 2).
- U = 4 and U = 2: `*_u4`, `*_u2`; only the leftover loop (nck < U): `left_only_u4`, `left_only_u2`; nck % U != 0 with fewer groups
  than waves (ngw = 0 on some waves): `few_groups_u4`, `few_groups_u2`; odd / even ngw: `odd_ngw_u4`, `even_ngw_u4`, `odd_ngw_u2`,
  `even_ngw_u2` (all with a leftover chunk).
- N % 16 != 0 and N % 4 != 0 (`rows*`, N = 50), N < 16 (`n7`), N = 1 (`n1`).
- nontemporal weight loads above 160e6 weight bytes: `nontemporal`; every other case streams with the default policy.
- static LDS at its largest (`lds_static_max`, nf * mt = 15) and dynamic LDS (`lds_dyn_16`, nf * mt = 16; `lds_dyn_max`, 6 x 5).
- MODE 2: K = 16384 exactly (`splitk_16384`), a ragged last slab (`splitk_ragged`), the smallest and the largest S of the grid
  (`splitk_smin`, `splitk_smax`), all at M % 16 != 0 (Mp / Np padding of the slabs).
- the hand-over at 128 / 129 rows: `route128` (k_skinny), `route129` (fp32: the LDS-tiled kernel; fp16: k_skinny).
- activations at the points where their expression changes (`test_linear_activation_edges`), scale / shift present or absent
  (`test_linear_scale_shift_forms` and, cyclically, every case of `test_linear_branch`).
- second call bit-equal, 0xFF outputs and workspaces with guard words behind both (every call), isolation of rows and columns
  (`test_linear_isolates_rows_and_columns`), a smaller shape in a used workspace (`test_linear_shrinking_in_a_used_workspace`).
- packing: `test_pack_rows_*`.
- the encoder: `test_encoder_stages` (MODE 0 through the device table and split-K, K = 1, 3, 9, B = 1 .. 80 on one handle),
  `test_encoder_member_ranges`, `test_encoder_smaller_batch_equals_fresh_handle`, `test_encoder_fold_edges`,
  `test_encoder_poisoned_workspace`.
- the mapping MLP: `test_classifier_chain`, `test_conditioner_mlp_tails`.

References: float64 on the GPU from the same fp32 inputs (fp16 forms: from fp16-rounded operands).  Every GEMM element's error is divided
by |scale_n| (|x| |w|^T)_mn + |shift_n| and must stay within GEMM_TOL; the activations are 1-Lipschitz or nearly so (GELU: 1.13), so the
post-activation error is held to the pre-activation bar; a stored fp16 activation gets F16_ROUND relative + F16_SUBNORMAL.  Where an
element misses that bar because the result itself is an fp32 number far larger than its pre-activation (softplus(u) near ln 2 at
|u| ~ 1e-3 would have to be exact to 1e-8, a sixth of its ulp), the fp32-relative rule of the earlier suites applies to those elements
(`assert_close`, ref32): over them, the kernel's worst error in ulps of the result must stay within max(1 ulp, 4 x the worst error of
torch's own fp32 evaluation of the same expression), both against float64; the measured ratios (at most 2.55) are in the
docstring of `assert_close`.  Exact paths
(packing, repeated calls, isolation, shrinking, untouched members) are compared bit for bit.

`nd_skinny_plan` reports neither the load policy nor the LDS form, so the `nt` and `dyn` fields of `skinny_plan` (160e6 weight bytes;
nd_skinny_red_bytes = 4 nf mt KiB against ND_SKINNY_STATIC_LDS = 60 KiB) cannot be cross-checked against the library: the coverage of
`nontemporal` and `lds_dyn_*` rests on the restatement of those two constants alone.

Not covered:
- S = 1 at K >= 16384 is reached only through many row groups (M = 1401 on 256 CUs: `splitk_smin`); with one row group the cost
  search of nd_skinny_launch_impl always cuts K while a slab stays 64 chunks deep.  On a CU count where the grid's smallest S is not 1,
  `splitk_smin` takes the smallest S the grid reaches.
- csrc/nd_persist.hip and MODE 1 (lin3 + lin4): the step-edge suite."""
import ctypes as Cty
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from oracle import ref_cpu
from test_gpu_grad_edges import check, poisoned, stream
from test_gpu_step_edges import F16_ROUND, F16_SUBNORMAL, GEMM_TOL, pick_mt

pytestmark = pytest.mark.gpu
DEV = "cuda"
BYTE_CAP = 256 * 1000 * 1000       # weights + workspace of one case
GUARD = 1024                       # 0xFF bytes kept behind every output and workspace, checked after the call
ACTS = ("none", "softplus", "relu", "gelu")
ACT_CODE = {"none": 0, "softplus": 1, "relu": 2, "gelu": 3}
CG_CAND = (1, 2, 3, 4, 6, 8, 12, 16)


def cdiv(a, b):
    return -(-a // b)


# ---- 1. the launch plan, restated ------------------------------------------------------------------------------------------------
def skinny_plan(K, N, M, nm, half, mode, ncu):
    """nd_skinny_launch_impl (csrc/nd_skinny_kernel.hpp): geometry, kernel instantiation, load policy and LDS form of one k_skinny launch."""
    mt = pick_mt(M)
    nfr, nch = cdiv(N, 16), (K // 32 if half else K // 16)
    mtiles, mgroups = cdiv(M, 16), cdiv(M, 16 * mt)
    wpm = min(max(ncu // nm, 1), nfr)
    while cdiv(nfr, wpm) > 6:
        wpm += 1
    S, cps = 1, nch
    if mode == 2:
        best, bw, bs = 1e30, wpm, 1
        for nfc in range(6, 0, -1):
            w = cdiv(nfr, nfc)
            wgs = nm * w * mgroups
            sc = 1 if wgs >= ncu else ncu // wgs
            while sc > 1 and nch // sc < 64:                     # every slab at least 64 chunks deep
                sc -= 1
            tot = wgs * sc
            util = tot / (float(ncu) * cdiv(tot, ncu)) if tot >= ncu else tot / float(ncu)
            cost = (1.0 + 0.3 * mt / (nfr / w)) / util
            if cost < best - 1e-9:
                best, bw, bs = cost, w, sc
        wpm, S = bw, bs
        cps = cdiv(nch, S)
        S = cdiv(nch, cps)
    nf = cdiv(nfr, wpm)
    U = 4 if mt <= 2 and nf <= 2 else 2
    last = nch - (S - 1) * cps                                   # chunks of the last slab
    lds = 4 * nf * mt * 1024
    return dict(K=K, N=N, M=M, nm=nm, half=half, mode=mode, mt=mt, nfr=nfr, nch=nch, mtiles=mtiles, mgroups=mgroups, wpm=wpm, nf=nf,
                rem=nfr % wpm, gx=nm * wpm, S=S, cps=cps, last=last, U=U, ngroups=cps // U, left=cps % U,
                nt=nm * N * float(K) * (2.0 if half else 4.0) > 160e6, dyn=lds > 60 * 1024, lds=lds)


def cond_gemm_plan(K, N, M, nm, half, ncu):
    """nd_cond_gemm_plan (csrc/nd_cond_gemm.hpp) for a [M, K] x [N, K] layer: use_tile and the k-slab workspace of its split tail."""
    use_tile = M > 128 and not half
    nfr, mfr, nch = cdiv(N, 16), cdiv(M, 16), K // 16
    tiles = nm * cdiv(mfr, 8) * cdiv(nfr, 8)
    if not use_tile:
        return dict(use_tile=False, ws_bytes=0)
    rem, split = tiles - tiles // ncu * ncu, 1
    if rem > 0:
        t_tile, best = nch * 64.0 * 32.0 / 2000.0, 1e30
        for s in CG_CAND:
            if s > 1 and (nch // s < 16 or rem * s > 512):
                continue
            t = (cdiv(rem * s, ncu) / s) * t_tile + (3.0 + rem * s * 65536.0 * 2.0 / 4.0e6 if s > 1 else 0.0)
            if t < best - 1e-9:
                best, split = t, s
    if split == 1:
        rem = 0
    return dict(use_tile=True, ws_bytes=rem * split * 128 * 128 * 4)


def linear_route(K, N, M, half, ncu):
    """linear_packed (csrc/nd_linear.hip): 'splitk' (k_skinny MODE 2 + k_splitk_epilogue) from K = 16384, else 'tile' (k_cond_gemm) above
    128 fp32 rows, else 'stream' (k_skinny MODE 0); with the launch plan of the streaming forms and the workspace nd_linear asks for."""
    el = 2 if half else 4
    packed = cdiv(M, 16) * 16 * K * el
    if K >= 16384:
        P = skinny_plan(K, N, M, 1, half, 2, ncu)
        extra = P["S"] * cdiv(M, 16) * 16 * cdiv(N, 16) * 16 * 4
        route = "splitk"
    else:
        cg = cond_gemm_plan(K, N, M, 1, half, ncu)
        P = None if cg["use_tile"] else skinny_plan(K, N, M, 1, half, 0, ncu)
        extra, route = cg["ws_bytes"], "tile" if cg["use_tile"] else "stream"
    return dict(route=route, plan=P, K=K, N=N, M=M, half=half, ws_bytes=packed + 256 + extra + 256,
                bytes=cdiv(N, 16) * 16 * K * el + packed + 512 + extra)


def library_skinny_plan(K, N, M, nm, half, mode):
    from nested_diffusion_amd import _lib
    lib = _lib.load()
    o = (Cty.c_int * 6)()
    _lib.check(lib.nd_skinny_plan(K, N, M, nm, int(half), mode, o), "nd_skinny_plan")
    return dict(gx=o[0], mgroups=o[1], S=o[2], nf=o[3], cps=o[4], threads=o[5], mt=lib.nd_skinny_row_fragments(M))


def assert_skinny_plan_matches_library(P):
    got = library_skinny_plan(P["K"], P["N"], P["M"], P["nm"], P["half"], P["mode"])
    want = dict({k: P[k] for k in ("gx", "mgroups", "S", "nf", "cps", "mt")}, threads=256)
    assert got == want, (P, got)


def assert_route_matches_library(R):
    from nested_diffusion_amd import _lib
    lib = _lib.load()
    assert lib.nd_linear_workspace_bytes(R["M"], R["K"], R["N"], int(R["half"])) == R["ws_bytes"], R
    if R["plan"] is not None:
        assert_skinny_plan_matches_library(R["plan"])
    else:                                                          # the tiled route: nd_step_plan reports use_tile for K = N only
        assert R["M"] > 128 and not R["half"]


# ---- 2. the branch search --------------------------------------------------------------------------------------------------------
ROWS = {1: 1, 16: 1, 17: 2, 32: 2, 33: 4, 64: 4, 65: 5, 80: 5, 81: 4, 128: 4}     # M -> MT
N_GRID = tuple(16 * n - 6 for n in range(1, 3400))                                  # N % 16 = 10: ragged last fragment, N % 4 != 0


def _p(want):
    """a predicate on the plan of a streaming route (None on the tiled route never matches)."""
    return lambda R: R["plan"] is not None and want(R["plan"], R)


def _chunks(u, cond):
    return dict(kc=tuple(range(1, 61)), Ns=(20,), Ms=(17,) if u == 4 else (40,),
                want=_p(lambda P, R: R["route"] == "stream" and P["U"] == u and cond(P["ngroups"], P["left"], P["nch"])))


def turns(ngroups):
    """ngw of the four waves of a workgroup: groups of U chunks are dealt to the waves in turn."""
    return [max(0, cdiv(ngroups - w, 4)) for w in range(4)]


def odd_turns(g):
    return any(t >= 3 and t % 2 == 1 for t in turns(g))             # a wave that ends on the lone MMA(wA) after the paired loop


def even_turns(g):
    return all(t >= 2 and t % 2 == 0 for t in turns(g))             # every wave ends inside the paired loop (the unused re-read of G(i + 2))


# every case: a grid (kc: K in chunks of 16 / 32 columns, or Ks: K itself) and the branch it must reach; the cheapest match is taken
LINEAR_CASES = {f"rows{M}": dict(kc=(11,), Ns=(50,), Ms=(M,), want=_p(lambda P, R, M=M, mt=mt: R["route"] == "stream" and P["mt"] == mt
                                 and (M not in (33, 81) or P["mgroups"] * P["mt"] > P["mtiles"])))
                for M, mt in ROWS.items()}
LINEAR_CASES.update({f"nf{v}": dict(kc=(5,), Ns=N_GRID, Ms=(19,), want=_p(lambda P, R, v=v: R["route"] == "stream" and P["nf"] == v
                                    and (P["rem"] != 0 if v > 1 else P["wpm"] == P["nfr"] > 1)))
                     for v in range(1, 7)})
LINEAR_CASES.update({
    "lds_static_max": dict(kc=(3,), Ns=N_GRID, Ms=(64, 70, 80), want=_p(lambda P, R: R["route"] == "stream" and P["nf"] * P["mt"] == 15
                                                                          and not P["dyn"])),
    "lds_dyn_16": dict(kc=(3,), Ns=N_GRID, Ms=(64, 70, 80), want=_p(lambda P, R: R["route"] == "stream" and P["nf"] * P["mt"] == 16
                                                                      and P["dyn"])),
    "lds_dyn_max": dict(kc=(3,), Ns=N_GRID, Ms=(64, 70, 80), want=_p(lambda P, R: R["route"] == "stream" and P["nf"] == 6 and P["mt"] == 5
                                                                       and P["dyn"] and P["rem"] != 0)),
    "left_only_u4": _chunks(4, lambda g, l, nch: g == 0 and nch == 3),
    "left_only_u2": _chunks(2, lambda g, l, nch: g == 0 and nch == 1),
    "few_groups_u4": _chunks(4, lambda g, l, nch: 0 < g < 4 and l != 0),
    "few_groups_u2": _chunks(2, lambda g, l, nch: 0 < g < 4 and l != 0),
    "odd_ngw_u4": _chunks(4, lambda g, l, nch: odd_turns(g) and g % 4 == 1 and l == 3),
    "even_ngw_u4": _chunks(4, lambda g, l, nch: even_turns(g) and l != 0),
    "odd_ngw_u2": _chunks(2, lambda g, l, nch: odd_turns(g) and g % 4 == 1 and l != 0),
    "even_ngw_u2": _chunks(2, lambda g, l, nch: even_turns(g) and l != 0),
    "n1": dict(kc=(7,), Ns=(1,), Ms=(17,), want=_p(lambda P, R: R["route"] == "stream")),
    "n7": dict(kc=(7,), Ns=(7,), Ms=(33,), want=_p(lambda P, R: R["route"] == "stream")),
    "nontemporal": dict(Ks=(16352,), Ns=tuple(range(2402, 5200, 50)), Ms=(19,), want=_p(lambda P, R: R["route"] == "stream" and P["nt"])),
    "splitk_16384": dict(Ks=(16384,), Ns=(20, 50), Ms=(17,), want=_p(lambda P, R: R["route"] == "splitk" and P["S"] > 1)),
    "splitk_ragged": dict(Ks=tuple(16384 + 32 * k for k in range(1, 41)), Ns=(50,), Ms=(33,),
                          want=_p(lambda P, R: R["route"] == "splitk" and P["S"] > 1 and P["last"] != P["cps"])),
    "splitk_partial": dict(Ks=(16384, 16416), Ns=N_GRID[:120], Ms=(19, 70), want=_p(lambda P, R: R["route"] == "splitk" and P["rem"] != 0
                                                                                     and P["nf"] > 1)),
    "route128": dict(kc=(9,), Ns=(50,), Ms=(128,), want=lambda R: R["route"] == "stream"),
    "route129": dict(kc=(9,), Ns=(50,), Ms=(129,), want=lambda R: R["route"] == ("stream" if R["half"] else "tile")),
})
SPLITK_GRID = dict(Ks=(16384, 16416, 32768, 65536, 131072, 262144, 524288), Ns=(10, 50, 106, 266, 1002, 4106),
                   Ms=(1, 17, 81, 129, 333, 641, 1401))


def search(ncu, half, want, kc=None, Ks=None, Ns=(), Ms=(), **_):
    """the cheapest (K, N, M) of the grid under the byte cap whose restated route satisfies `want` at `ncu` CUs."""
    Ks = Ks if Ks is not None else tuple(c * (32 if half else 16) for c in kc)
    for K, M in sorted(((K, M) for K in Ks for M in Ms), key=lambda km: km[0] * km[1]):
        for N in Ns:                                               # ascending: the first match is the cheapest of this (K, M)
            R = linear_route(K, N, M, half, ncu)
            if R["bytes"] > BYTE_CAP:
                break
            if want(R):
                return R
    raise AssertionError(f"no shape of the grid reaches the branch on {ncu} CUs")


def splitk_extremes(ncu, half):
    """the shapes of SPLITK_GRID under the cap with the smallest and the largest S, both at M % 16 != 0 (cheapest on ties)."""
    found = []
    for K in SPLITK_GRID["Ks"]:
        for N in SPLITK_GRID["Ns"]:
            for M in SPLITK_GRID["Ms"]:
                R = linear_route(K, N, M, half, ncu)
                if R["bytes"] <= BYTE_CAP and M % 16 != 0:
                    found.append((R["plan"]["S"], R["bytes"], R))
    assert found, f"no split-K shape under the cap on {ncu} CUs"
    smin = min(found, key=lambda t: (t[0], t[1]))[2]
    smax = min(found, key=lambda t: (-t[0], t[1]))[2]
    assert smin["plan"]["S"] < smax["plan"]["S"]
    return {"splitk_smin": smin, "splitk_smax": smax}


def all_linear_shapes(ncu):
    """every case of LINEAR_CASES and the two split-K extremes, per operand type, resolved at `ncu` CUs: (name, half) -> route."""
    out = {}
    for half in (False, True):
        for name, spec in LINEAR_CASES.items():
            out[name, half] = search(ncu, half, **spec)
        for name, R in splitk_extremes(ncu, half).items():
            out[name, half] = R
    return out


def check_linear_coverage(shapes):
    """the branches of section (b) over the resolved shapes, per operand type."""
    for half in (False, True):
        Rs = {n: R for (n, h), R in shapes.items() if h == half}
        Ps = [R["plan"] for R in Rs.values() if R["plan"] is not None]
        m0 = [P for P in Ps if P["mode"] == 0]
        m2 = [P for P in Ps if P["mode"] == 2]
        assert {P["mt"] for P in m0} == {1, 2, 4, 5} and {P["M"] for P in m0} >= set(ROWS)
        assert any(P["mgroups"] * P["mt"] > P["mtiles"] and P["mgroups"] > 1 for P in m0)             # clamped xp[mt], last of two groups
        for v in range(2, 7):
            assert any(P["nf"] == v and P["rem"] != 0 for P in m0), v
        assert any(P["nf"] == 1 for P in m0) and any(P["nf"] > 1 and P["rem"] != 0 for P in m2)
        for U in (4, 2):
            pu = [P for P in m0 if P["U"] == U]
            assert any(P["ngroups"] == 0 for P in pu) and any(0 < P["ngroups"] < 4 and P["left"] for P in pu), U
            assert any(odd_turns(P["ngroups"]) and P["left"] for P in pu) and any(even_turns(P["ngroups"]) and P["left"] for P in pu), U
        assert any(P["N"] == 1 for P in m0) and any(1 < P["N"] < 16 for P in m0) and any(P["N"] % 16 and P["N"] % 4 for P in m0)
        assert any(P["nt"] for P in m0) and any(not P["nt"] for P in m0)
        assert any(P["dyn"] and P["nf"] * P["mt"] == 16 for P in m0) and any(P["lds"] == 120 * 1024 for P in m0)
        assert any(not P["dyn"] and P["lds"] == 60 * 1024 for P in m0)
        assert any(P["K"] == 16384 for P in m2) and any(P["last"] != P["cps"] for P in m2) and all(P["M"] % 16 for P in m2)
        assert len({P["S"] for P in m2}) >= 3
        assert Rs["route128"]["route"] == "stream" and Rs["route129"]["route"] == ("stream" if half else "tile")
        assert all(R["bytes"] <= BYTE_CAP for R in Rs.values())


def slabs_reserved(D):
    """the k-slabs `carve` (csrc/nd_handle.hip) reserves per member for the encoder's split-K first layer."""
    return D // 16 // 64 + 1


def assert_encoder_slabs_fit(D, H, B, nm, half, ncu=None):
    """S of the multi-member MODE 2 launch nd_encode makes at (B, nm) never exceeds the slabs reserved at load; ncu None: the
    library's own plan (current device, or 256 without one), else the restated plan at that CU count."""
    S = library_skinny_plan(D, H, B, nm, half, 2)["S"] if ncu is None else skinny_plan(D, H, B, nm, half, 2, ncu)["S"]
    assert 1 <= S <= slabs_reserved(D), (D, H, B, nm, half, ncu, S)
    return S


@functools.lru_cache(None)
def ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(None)
def device_shapes():
    return all_linear_shapes(ncu())


def test_plan_restatement_matches_library_at_device_cu_count():
    """every case shape against nd_skinny_plan / nd_skinny_row_fragments / nd_linear_workspace_bytes at this device's CU count, the
    coverage of section (b) over them, and a wider sweep of the restated plan."""
    torch.zeros(1, device=DEV)
    shapes = device_shapes()
    for R in shapes.values():
        assert_route_matches_library(R)
    check_linear_coverage(shapes)
    sweep_plans(ncu())


def sweep_plans(ncu_):
    for half in (False, True):
        for K in (32, 96, 4096, 16352, 16384, 16416, 150528):
            for N in (1, 50, 272, 4106, 20490):
                for M in (1, 17, 64, 70, 81, 128, 129, 640):
                    assert_route_matches_library(linear_route(K, N, M, half, ncu_))
                    for nm in (3, 9):
                        for mode in (0, 2):
                            assert_skinny_plan_matches_library(skinny_plan(K, N, M, nm, half, mode, ncu_))


# ---- 3. helpers ------------------------------------------------------------------------------------------------------------------
def lib():
    from nested_diffusion_amd import _lib
    return _lib.load()


def poison_bytes(n):
    return torch.full((n,), 0xFF, dtype=torch.uint8, device=DEV)


def guarded(nbytes):
    """(whole, view): `nbytes` 0xFF bytes at a 256-byte aligned address with GUARD more behind them."""
    whole = poison_bytes(nbytes + GUARD + 256)
    off = (-whole.data_ptr()) % 256
    return whole, whole[off:off + nbytes]


def assert_guard_intact(whole, view, what):
    off = view.data_ptr() - whole.data_ptr()
    tail = whole[off + view.numel():]
    assert bool((tail == 0xFF).all()), f"{what}: bytes behind the buffer were written"
    assert bool((whole[:off] == 0xFF).all()), f"{what}: bytes before the buffer were written"


def rnd(shape, seed, scale=1.0, uniform=False):
    g = torch.Generator(device=DEV).manual_seed(seed)
    if uniform:
        return (torch.rand(shape, generator=g, device=DEV) * 2 - 1) * scale
    return torch.randn(shape, generator=g, device=DEV) * scale


def pack(w, half, R=None, K=None):
    """nd_pack_rows into a guarded 0xFF buffer: the packed image as a uint8 tensor."""
    R, K = (w.shape if R is None else (R, K))
    n = lib().nd_packed_bytes(R, K, int(half))
    assert n == cdiv(R, 16) * 16 * K * (2 if half else 4)
    whole, view = guarded(n)
    check(lib().nd_pack_rows(w.data_ptr(), view.data_ptr(), R, K, int(half), stream()), "nd_pack_rows")
    torch.cuda.synchronize()
    assert_guard_intact(whole, view, "nd_pack_rows")
    return view


def linear_abi(x, wpk, scale, shift, act, N, half, ws=None):
    """nd_linear through the C ABI into a guarded 0xFF output, on a guarded 0xFF workspace of exactly the bytes the library asks for
    (or `ws`, a (whole, view) pair used before)."""
    M, K = x.shape
    need = lib().nd_linear_workspace_bytes(M, K, N, int(half))
    assert need > 0
    ws_whole, ws_view = ws if ws is not None else guarded(need)
    assert ws_view.numel() >= need
    o_whole, o_view = guarded(M * N * 4)
    check(lib().nd_linear(x.data_ptr(), wpk.data_ptr(), None if scale is None else scale.data_ptr(), None if shift is None else shift.data_ptr(),
                          o_view.data_ptr(), M, K, N, ACT_CODE[act], int(half), ws_view.data_ptr(), need, stream()), "nd_linear")
    torch.cuda.synchronize()
    assert_guard_intact(o_whole, o_view, "nd_linear output")
    assert_guard_intact(ws_whole, ws_view[:need] if ws is None else ws_view, "nd_linear workspace")
    return o_view.view(torch.float32).reshape(M, N)


def act64(u, act):
    if act == "softplus":
        return Fn.softplus(u)
    if act == "relu":
        return torch.relu(u)
    if act == "gelu":
        return Fn.gelu(u)
    return u


def operand64(t, half):
    return (t.half() if half else t).double()


def linear_ref(x, w, scale, shift, act, half):
    """float64 reference and the per-element bar |scale| (|x| |w|^T) + |shift| of act(scale * x w^T + shift)."""
    xd, wd = operand64(x, half), operand64(w, half)
    u, bar = xd @ wd.T, xd.abs() @ wd.abs().T
    if scale is not None:
        u, bar = u * scale.double(), bar * scale.double().abs()
    if shift is not None:
        u, bar = u + shift.double(), bar + shift.double().abs()
    return act64(u, act), bar


def linear_ref32(x, w, scale, shift, act, half):
    """torch's own fp32 evaluation of the same expression (the fp32-relative rule of assert_close)."""
    x, w = (x.half().float(), w.half().float()) if half else (x, w)
    u = x @ w.T
    if scale is not None:
        u = u * scale
    if shift is not None:
        u = u + shift
    return act64(u, act)


def ulp32(ref):
    """the spacing of fp32 numbers at |ref| (float64 tensor)."""
    a = ref.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))).double() - a.double())


WORST = {}
FP32_RULE = {}                    # key -> (kernel ulps, torch fp32 ulps) over the elements judged by the fp32-relative rule


def assert_close(got, ref, bar, what, rounding=0.0, ref32=None):
    """|got - ref| <= GEMM_TOL * bar + rounding * |ref| (+ the fp16 subnormal floor) per element; NaN fails.
    ref32 (a callable giving torch's fp32 result for the same inputs): the elements that miss the bar are judged by the fp32-relative
    rule instead -- their worst error in fp32 ulps of the result must stay within max(1, 4 x torch fp32's worst error over the same
    elements), both against float64.  Only softplus / GELU outputs whose pre-activation is far smaller than the result get there.
    Measured on an MI355X, worst kernel error : worst torch fp32 error over those elements, in ulps of the result (printed at the end
    of the module): test_linear_branch 2.10 : 0.95 (ratio 2.21) fp32 and 2.17 : 0.86 (2.51) fp16; test_linear_scale_shift_forms
    1.70 : 0.66 (2.55) and 1.89 : 0.83 (2.27); test_linear_activation_edges (softplus(0) at a zero bar) 0.03 : 0.03 (1.00).  No encoder
    or GELU element misses the plain bar."""
    got = got.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    slack = rounding * ref.abs() + (F16_SUBNORMAL if rounding else 0.0)
    err = ((got - ref).abs() - slack).clamp_min(0) / bar.clamp_min(1e-300)
    bad = ~(err <= GEMM_TOL)
    if bool(bad.any()) and ref32 is not None:
        u = ulp32(ref)[bad]
        e_k = float(((got - ref).abs()[bad] / u).max())
        e_t = float(((ref32().double() - ref).abs()[bad] / u).max())
        key = what.split(":")[0]
        if e_k <= max(1.0, 4.0 * e_t):                             # NaN fails
            old = FP32_RULE.get(key, (0.0, 0.0))
            FP32_RULE[key] = max(old, (e_k, e_t))
            err = torch.where(bad, torch.zeros_like(err), err)
            bad = torch.zeros_like(bad)
        else:
            what = f"{what} [fp32 rule: kernel {e_k:.3g} ulp, torch fp32 {e_t:.3g} ulp over {int(bad.sum())} elements]"
    if bool(bad.any()):
        idx = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements off the bar {GEMM_TOL:g}, first at {idx}: got "
                             f"{float(got[idx])}, want {float(ref[idx])}, bar scale {float(bar[idx])}; rows hit "
                             f"{bad.any(1).nonzero().flatten()[:8].tolist()}, columns hit {bad.any(0).nonzero().flatten()[:8].tolist()}")
    key = what.split(":")[0]
    WORST[key] = max(WORST.get(key, 0.0), float(err.max()))


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def linear_inputs(R, seed, forms="both"):
    K, N, M = R["K"], R["N"], R["M"]
    x = rnd((M, K), seed)
    w = rnd((N, K), seed + 1, 1.0 / math.sqrt(K), uniform=True)
    scale = rnd((N,), seed + 2) if forms in ("both", "scale") else None
    shift = rnd((N,), seed + 3) if forms in ("both", "shift") else None
    return x, w, scale, shift


FORMS = ("both", "scale", "shift", "neither")


# ---- (a) packing -----------------------------------------------------------------------------------------------------------------
def pk_index(R, K, half):
    """nd_pk (float index) / nd_pkh (half index) of every (r, k) of an [R, K] matrix, restated: int64 [R, K]."""
    r, k = np.meshgrid(np.arange(R, dtype=np.int64), np.arange(K, dtype=np.int64), indexing="ij")
    if half:
        return ((r >> 4) * (K // 32) + (k >> 5)) * 512 + ((r & 15) + 16 * ((k & 31) >> 3)) * 8 + (k & 7)
    return ((r >> 4) * (K // 16) + (k >> 4)) * 256 + ((r & 15) + 16 * ((k & 15) >> 2)) * 4 + (k & 3)


def expected_image(src, half):
    """the packed image of a numpy fp32 [R, K]: raw words (uint32 / uint16) with the pad rows zero."""
    R, K = src.shape
    vals = src.astype(np.float16).view(np.uint16) if half else src.view(np.uint32)       # numpy rounds to nearest even, overflow to inf
    img = np.zeros(cdiv(R, 16) * 16 * K, dtype=vals.dtype)
    img[pk_index(R, K, half).ravel()] = vals.ravel()
    return img


def assert_pack_exact(src, half):
    got = pack(src, half).cpu().numpy().view(np.uint16 if half else np.uint32)
    with np.errstate(over="ignore"):
        want = expected_image(src.cpu().numpy(), half)
    assert got.shape == want.shape
    if not np.array_equal(got, want):
        i = int(np.nonzero(got != want)[0][0])
        raise AssertionError(f"packed image differs at word {i} of {want.size}: got {got[i]:#x}, want {want[i]:#x} (R={src.shape[0]}, K={src.shape[1]}, half={half})")


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("R", [1, 15, 16, 17, 33])
def test_pack_rows_layout_and_zeroed_pad_rows(R, half):
    """nd_pack_rows bit for bit against nd_pk / nd_pkh restated in numpy, into 0xFF destinations: rows R .. 16 ceil(R/16) read as zeros."""
    unit = 32 if half else 16
    for kc in (1, 2, 5, 13):
        assert_pack_exact(rnd((R, kc * unit), 100 + R + kc), half)


@pytest.mark.parametrize("half", [False, True])
def test_pack_rows_grid_stride_loop_runs_twice(half):
    """one image above 8192 * 256 sixteen-byte pieces: the grid-stride loops of k_pack_rows / k_pack_rows_h take a second trip."""
    R, K = 33, (32 * 10924 if half else 16 * 10923)
    assert cdiv(R, 16) * 16 * K * (2 if half else 4) // 16 > 8192 * 256
    assert_pack_exact(rnd((R, K), 7), half)


def test_pack_rows_fp16_rounding_edges():
    """ties to even, the largest finite value, values that round up to infinity (65520), subnormals and their ties, signed zeros."""
    vals = [65504.0, 65519.996, 65520.0, 65536.0, 1e9, float("inf"), 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -20), 3 * 2.0 ** -25,
            2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -20, 2049.0, 2051.0, 0.0, 1e-10,
            0.1, 1 / 3]
    src = torch.tensor(vals + [-v for v in vals], dtype=torch.float32)
    src = torch.cat([src, torch.zeros(64 - src.numel() % 64)]).reshape(-1, 32).to(DEV)
    want = src.cpu().numpy().astype(np.float16)
    assert np.isinf(want.ravel()[2]) and want.ravel()[0] == 65504 and want.ravel()[1] == 65504 and want.ravel()[7] == 0 and want.ravel()[8] > 0
    assert_pack_exact(src, True)


def test_packed_bytes_restated():
    for R in (1, 15, 16, 17, 33, 4106):
        for K in (16, 32, 48, 64, 16384, 150528):
            assert lib().nd_packed_bytes(R, K, 0) == cdiv(R, 16) * 16 * K * 4
            assert lib().nd_packed_bytes(R, K, 1) == (cdiv(R, 16) * 16 * K * 2 if K % 32 == 0 else 0)
    for R, K, dt in ((0, 16, 0), (-1, 16, 0), (1, 0, 0), (1, 8, 0), (1, 24, 0), (1, 16, 1), (1, 48, 1), (1, 32, 2), (1, 32, -1)):
        assert lib().nd_packed_bytes(R, K, dt) == 0, (R, K, dt)


# ---- (b) nd_linear ---------------------------------------------------------------------------------------------------------------
CASE_NAMES = list(LINEAR_CASES) + ["splitk_smin", "splitk_smax"]


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("case", CASE_NAMES)
def test_linear_branch(case, half, record_property):
    """one named case per branch (see the module docstring): float64 reference with the per-element bar, 0xFF output and workspace with
    guard bytes, the plan cross-checked against the library, a second call bit-equal."""
    R = device_shapes()[case, half]
    assert_route_matches_library(R)
    record_property("shape", {k: (R["plan"] or {}).get(k) for k in ("K", "N", "M", "mt", "nf", "rem", "U", "ngroups", "left", "S", "cps", "last")})
    i = CASE_NAMES.index(case)
    act, forms = ACTS[i % 4], FORMS[(i // 4 + i) % 4]
    x, w, scale, shift = linear_inputs(R, 1000 + 10 * i + half, forms)
    wpk = pack(w, half)
    out = linear_abi(x, wpk, scale, shift, act, R["N"], half)
    ref, bar = linear_ref(x, w, scale, shift, act, half)
    assert_close(out, ref, bar, f"{R['route']}{'/fp16' if half else ''}: {case} K={R['K']} N={R['N']} M={R['M']} act={act} {forms}",
                 ref32=lambda: linear_ref32(x, w, scale, shift, act, half))
    assert same_bits(out, linear_abi(x, wpk, scale, shift, act, R["N"], half)), "a second call differs"


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("case", ["rows17", "splitk_16384"])
def test_linear_activation_edges(case, half):
    """pre-activations placed exactly (zero weight rows, the value in `shift`): softplus round its threshold of 20 and far below 0, ReLU
    at exactly +-0, GELU tails; the other columns carry random values scaled into the same ranges."""
    R = device_shapes()[case, half]
    points = [19.0, 19.999998, 20.0, 20.000002, 21.0, 30.0, 88.0, -1.0, -20.0, -87.0, -104.0, -200.0, 0.0, -0.0, 1e-30, -1e-30, 5.0, -5.0,
              -6.0, -9.0, -13.0, -40.0, 40.0, 0.9277, -0.9277, 1.312, -1.312]
    N, K, M = len(points) + 23, R["K"], R["M"]
    x = rnd((M, K), 5)
    w = rnd((N, K), 6, 8.0 / math.sqrt(K))
    w[: len(points)] = 0.0
    shift = rnd((N,), 7, 10.0)
    shift[: len(points)] = torch.tensor(points, device=DEV)
    wpk = pack(w, half)
    assert linear_route(K, N, M, half, ncu())["route"] == R["route"]
    for act in ACTS:
        out = linear_abi(x, wpk, None, shift, act, N, half)
        ref, bar = linear_ref(x, w, None, shift, act, half)
        assert_close(out, ref, bar, f"act edges {act}: {case}{'/fp16' if half else ''}",
                     ref32=lambda: linear_ref32(x, w, None, shift, act, half))
        exact = act64(shift[: len(points)].double(), act).float().expand(M, -1) if act in ("none", "relu") else None
        if exact is not None:                                        # x . 0 + shift: the identity and ReLU are exact
            assert torch.equal(out[:, : len(points)], exact)
        if act == "softplus":                                        # above the threshold softplus is the identity, bit for bit
            big = [j for j, v in enumerate(points) if v > 20.0]
            assert torch.equal(out[:, big], shift[big].expand(M, -1))


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("forms", FORMS)
@pytest.mark.parametrize("case", ["rows65", "nf3", "splitk_ragged"])
def test_linear_scale_shift_forms(case, forms, half):
    R = device_shapes()[case, half]
    x, w, scale, shift = linear_inputs(R, 300 + FORMS.index(forms), forms)
    out = linear_abi(x, pack(w, half), scale, shift, "softplus", R["N"], half)
    ref, bar = linear_ref(x, w, scale, shift, "softplus", half)
    assert_close(out, ref, bar, f"forms {forms}: {case}{'/fp16' if half else ''}",
                 ref32=lambda: linear_ref32(x, w, scale, shift, "softplus", half))


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("case", ["rows81", "nf4", "lds_dyn_max", "odd_ngw_u4", "few_groups_u2", "splitk_ragged", "splitk_partial", "splitk_smax"])
def test_linear_isolates_rows_and_columns(case, half):
    """one x row all NaN: only that output row may differ; one weight row all NaN: only that output column may differ; every other element
    is bit-equal to the clean run (no reduction or epilogue mixes rows, fragments or slabs)."""
    R = device_shapes()[case, half]
    x, w, scale, shift = linear_inputs(R, 77)
    M, N = R["M"], R["N"]
    clean = linear_abi(x, pack(w, half), scale, shift, "softplus", N, half)
    assert bool(torch.isfinite(clean).all())
    for r in sorted({0, M // 2, M - 1}):
        xn = x.clone()
        xn[r] = float("nan")
        got = linear_abi(xn, pack(w, half), scale, shift, "softplus", N, half)
        keep = torch.arange(M, device=DEV) != r
        assert same_bits(got[keep], clean[keep]), f"a NaN in x row {r} reached another row"
        assert bool(torch.isnan(got[r]).all())
    for n in sorted({0, N // 2, N - 1}):
        wn = w.clone()
        wn[n] = float("nan")
        got = linear_abi(x, pack(wn, half), scale, shift, "softplus", N, half)
        keep = torch.arange(N, device=DEV) != n
        assert same_bits(got[:, keep], clean[:, keep]), f"a NaN in weight row {n} reached another column"
        assert bool(torch.isnan(got[:, n]).all())


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("big,small", [("splitk_smax", "splitk_ragged"), ("splitk_smax", "rows17"), ("lds_dyn_max", "rows1"),
                                       ("route129", "rows81"), ("splitk_smax", "splitk_smin")])
def test_linear_shrinking_in_a_used_workspace(big, small, half):
    """after a large call, a smaller shape in the same workspace gives the bits it gives in a fresh 0xFF workspace."""
    Rb, Rs = device_shapes()[big, half], device_shapes()[small, half]
    if Rs["ws_bytes"] > Rb["ws_bytes"]:
        Rb, Rs = Rs, Rb
    ws = guarded(Rb["ws_bytes"])
    xb, wb, scb, shb = linear_inputs(Rb, 11)
    linear_abi(xb, pack(wb, half), scb, shb, "none", Rb["N"], half, ws=ws)
    xs, w_s, scs, shs = linear_inputs(Rs, 12)
    wpk = pack(w_s, half)
    used = linear_abi(xs, wpk, scs, shs, "gelu", Rs["N"], half, ws=ws)
    fresh = linear_abi(xs, wpk, scs, shs, "gelu", Rs["N"], half)
    assert same_bits(used, fresh)
    ref, bar = linear_ref(xs, w_s, scs, shs, "gelu", half)
    assert_close(used, ref, bar, f"shrink: {big} -> {small}", ref32=lambda: linear_ref32(xs, w_s, scs, shs, "gelu", half))


# ---- (c) the encoder hoist -------------------------------------------------------------------------------------------------------
ENC_T, ENC_C = 2, 2
ENC_DIMS = {False: dict(H=48, F=80), True: dict(H=96, F=160)}          # unequal, no multiples of 64; fp32: H % 32 == 16
ENC_BATCHES = (80, 1, 15, 16, 17, 33, 70, 80)


def ragged_splitk_dim(half, H, B, nm):
    """the smallest data_dim = 16384 + 32 k whose split-K launch at (B, nm) has a ragged last slab."""
    for k in range(1, 200):
        P = skinny_plan(16384 + 32 * k, H, B, nm, half, 2, ncu())
        if P["S"] > 1 and P["last"] != P["cps"]:
            return P["K"]
    raise AssertionError("no ragged split-K data_dim found")


def enc_data_dim(kind, half, K):
    H = ENC_DIMS[half]["H"]
    return {"mode0": 352, "splitk": 16384}.get(kind) or ragged_splitk_dim(half, H, 33, K)


def enc_members(D, H, F, K, seed):
    return [ref_cpu.init_cond_model_params(D, H, F, ENC_C, ENC_T, True, seed=seed + k) for k in range(K)]


def enc_engine(D, H, F, K, max_batch, half, members, fill=None):
    from nested_diffusion_amd.engine import EnsembleEngine
    eng = EnsembleEngine(ENC_C, D, H, F, ENC_T, n_members=K, max_batch=max_batch, max_rows=max_batch, dtype="f16" if half else "f32")
    if fill is not None:
        eng.workspace.fill_(fill)
        base = (eng.workspace.data_ptr() + 255) & ~255
        check(eng.lib.nd_bind_workspace(eng.h, base, eng.lib.nd_workspace_bytes(Cty.byref(eng.cfg))), "nd_bind_workspace")
    for k, p in enumerate(members):
        eng.load_member(k, p)
    return eng


def enc_params64(p):
    return {k: v.to(DEV, torch.float64) for k, v in p.items() if v.is_floating_point()}


def enc_stage64(P, lin, bn, h, half, act):
    """act(BN(W h + b)) in float64 by the reference's BatchNorm formula (eps 1e-5) and the bar |s| (|h| |W|^T) + |s b + beta - mean s|,
    s = bn.weight / sqrt(var + eps); fp16 handles stream W and h as fp16."""
    W = P[lin + ".weight"]
    if half:
        W, h = W.float().half().double(), h.float().half().double()
    u = ref_cpu._bn_eval(Fn.linear(h, W, P[lin + ".bias"]), P, bn)
    s = P[bn + ".weight"] / torch.sqrt(P[bn + ".running_var"] + ref_cpu.BN_EPS)
    c = s * P[lin + ".bias"] + (P[bn + ".bias"] - P[bn + ".running_mean"] * s)
    return act64(u, act), (h.abs() @ W.abs().T) * s.abs() + c.abs()


def enc_stage32(P, lin, bn, h, half, act):
    """torch's own fp32 evaluation of the same stage."""
    P32 = {k: P[k].float() for k in (lin + ".weight", lin + ".bias", bn + ".weight", bn + ".bias", bn + ".running_mean", bn + ".running_var")}
    W, h = P32[lin + ".weight"], h.float()
    if half:
        W, h = W.half().float(), h.half().float()
    return act64(ref_cpu._bn_eval(Fn.linear(h, W, P32[lin + ".bias"]), P32, bn), act)


def encode(eng, x, member0=0, n_members=None):
    """EnsembleEngine.encode; on a split-K handle first the slab inequality at this (B, nm): S of the launch <= the slabs reserved."""
    nm = eng.K - member0 if n_members is None else n_members
    if eng.D >= 16384:
        assert_encoder_slabs_fit(eng.D, eng.H, x.shape[0], nm, eng.dtype == 1)
    eng.encode(x, member0=member0, n_members=nm)


def read_stages(eng, k, B):
    """e0, e1 (nd_member_buffer which = 3, 4: [B, H]) and xe (which = 0: [B, F]) through the C ABI into 0xFF buffers."""
    outs = []
    for which, width in ((3, eng.H), (4, eng.H), (0, eng.F)):
        t = poisoned(B, width)
        check(eng.lib.nd_member_buffer(eng.h, k, which, t.data_ptr(), B, stream()), "nd_member_buffer")
        outs.append(t)
    torch.cuda.synchronize()
    assert all(not bool(torch.isnan(t).any()) for t in outs), "an element of e0 / e1 / xe was not written"
    return tuple(outs)


def check_encoder_stages(eng, P, k, x, what):
    """stage-local: e0 from x, e1 from the kernel's own e0, xe from the kernel's own e1."""
    half = eng.dtype == 1
    B = x.shape[0]
    e0, e1, xe = read_stages(eng, k, B)
    rounding = F16_ROUND if half else 0.0
    ref, bar = enc_stage64(P, "encoder_x.0", "encoder_x.1", x.double(), half, "softplus")
    assert bool(torch.isfinite(ref).all())
    assert_close(e0, ref, bar, f"e0{'/fp16' if half else ''}: {what} member {k}", rounding,
                 ref32=lambda: enc_stage32(P, "encoder_x.0", "encoder_x.1", x, half, "softplus"))
    ref, bar = enc_stage64(P, "encoder_x.3", "encoder_x.4", e0.double(), half, "softplus")
    assert_close(e1, ref, bar, f"e1{'/fp16' if half else ''}: {what} member {k}", rounding,
                 ref32=lambda: enc_stage32(P, "encoder_x.3", "encoder_x.4", e0, half, "softplus"))
    ref, bar = enc_stage64(P, "encoder_x.6", "norm", e1.double(), half, "none")
    assert bool(torch.isfinite(ref).all())
    assert_close(xe, ref, bar, f"xe{'/fp16' if half else ''}: {what} member {k}")
    return e0, e1, xe


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("K", [1, 3, 9])
@pytest.mark.parametrize("kind", ["mode0", "splitk", "splitk_ragged"])
def test_encoder_stages(kind, K, half):
    """e0, e1 and xe of every member, stage by stage, at B = 80, 1, 15, 16, 17, 33, 70, 80 on one handle with max_batch = 80;
    data_dim below 16384 (MODE 0 through the device table), 16384 and a ragged split-K depth; K = 9 exceeds the inline descriptors."""
    H, F = ENC_DIMS[half]["H"], ENC_DIMS[half]["F"]
    D = enc_data_dim(kind, half, K)
    assert (D >= 16384) == (kind != "mode0") and (half or H % 32 == 16) and H != F and H % 64 and F % 64
    members = enc_members(D, H, F, K, 40)
    Ps = [enc_params64(p) for p in members]
    eng = enc_engine(D, H, F, K, 80, half, members)
    xs = rnd((80, D), 3).abs()
    for B in ENC_BATCHES:
        x = xs[:B].contiguous()
        encode(eng, x)
        for which in (3, 4):                                       # the Python wrapper allocates [rows, H] and returns the same bits
            t = eng.member_buffer(K - 1, which, B)
            assert t.shape == (B, H) and same_bits(t, read_stages(eng, K - 1, B)[which - 3])
        for k in range(K):
            check_encoder_stages(eng, Ps[k], k, x, f"{kind} D={D} K={K} B={B}")
    if kind == "splitk_ragged":
        P = skinny_plan(D, H, 33, K, half, 2, ncu())
        assert P["last"] != P["cps"]


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("kind", ["mode0", "splitk_ragged"])
def test_encoder_member_ranges(kind, half):
    """ranges with member0 > 0 and n_members < K on a K = 9 handle: the members of the range follow the new batch, every other member
    keeps its earlier e0, e1 and xe bit for bit."""
    H, F, K = ENC_DIMS[half]["H"], ENC_DIMS[half]["F"], 9
    D = enc_data_dim(kind, half, 3)
    members = enc_members(D, H, F, K, 60)
    Ps = [enc_params64(p) for p in members]
    eng = enc_engine(D, H, F, K, 40, half, members)
    x1, x2 = rnd((33, D), 8).abs(), rnd((17, D), 9).abs()
    encode(eng, x1)
    before = [read_stages(eng, k, 33) for k in range(K)]
    for m0, nm in ((2, 3), (8, 1), (1, 7)):
        encode(eng, x2, m0, nm)
        for k in range(K):
            if m0 <= k < m0 + nm:
                check_encoder_stages(eng, Ps[k], k, x2, f"range [{m0},{m0 + nm}) {kind}")
            else:
                for a, b in zip(read_stages(eng, k, 33), before[k]):
                    assert same_bits(a, b), f"member {k} outside [{m0},{m0 + nm}) changed"
        encode(eng, x1)                                             # all members back on the first batch
        for k in range(K):
            for a, b in zip(read_stages(eng, k, 33), before[k]):
                assert same_bits(a, b)


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("kind", ["mode0", "splitk", "splitk_ragged"])
def test_encoder_smaller_batch_equals_fresh_handle(kind, half):
    """B below max_batch after a larger B gives the bits of a fresh handle that only saw the smaller B (stale rows of the packed batch,
    of e0 / e1 and of the split-K slabs are not read)."""
    H, F, K = ENC_DIMS[half]["H"], ENC_DIMS[half]["F"], 3
    D = enc_data_dim(kind, half, K)
    members = enc_members(D, H, F, K, 70)
    xs = rnd((80, D), 4).abs()
    eng = enc_engine(D, H, F, K, 80, half, members)
    encode(eng, xs)
    for B in (1, 15, 17, 33, 70):
        encode(eng, xs[:B].contiguous())
        fresh = enc_engine(D, H, F, K, 80, half, members, fill=0xFF)
        encode(fresh, xs[:B].contiguous())
        for k in range(K):
            for a, b in zip(read_stages(eng, k, B), read_stages(fresh, k, B)):
                assert same_bits(a, b), (kind, B, k)
        del fresh
        encode(eng, xs)


def fold_edge_members(D, H, F, K, seed):
    """negative BatchNorm weights, running variance 0 and 1e-12, a large running mean, zero bias: in all three folded layers."""
    members = enc_members(D, H, F, K, seed)
    for p in members:
        for bn, lin, n in (("encoder_x.1", "encoder_x.0", H), ("encoder_x.4", "encoder_x.3", H), ("norm", "encoder_x.6", F)):
            p[bn + ".weight"][0::4] *= -1.0
            p[bn + ".running_var"][1::8] = 0.0
            p[bn + ".running_var"][2::8] = 1e-12
            p[bn + ".weight"][1::8] *= 0.01                        # (s = w / sqrt(eps) = 316 w there: kept small so that an fp16 handle's
            p[bn + ".weight"][2::8] *= 0.01                        #  stored activations stay below 65504)
            p[bn + ".running_mean"][3::8] = 1000.0
            p[bn + ".running_mean"][5::8] = -1000.0
            p[lin + ".bias"][0::3] = 0.0
            p[bn + ".bias"][4::8] = 0.0
    return members


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("kind", ["mode0", "splitk"])
def test_encoder_fold_edges(kind, half):
    """k_fold_bn at its edges (see fold_edge_members); the float64 reference stays finite and the stage bars hold."""
    H, F, K = ENC_DIMS[half]["H"], ENC_DIMS[half]["F"], 2
    D = enc_data_dim(kind, half, K)
    members = fold_edge_members(D, H, F, K, 90)
    eng = enc_engine(D, H, F, K, 33, half, members)
    x = rnd((33, D), 2).abs()
    encode(eng, x)
    for k in range(K):
        check_encoder_stages(eng, enc_params64(members[k]), k, x, f"fold edges {kind}")


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("kind", ["mode0", "splitk_ragged"])
def test_encoder_poisoned_workspace(kind, half):
    """the handle workspace as 0xFF bytes before nd_load_member, and again before a second run everywhere the load does not own.
    Run 1: the whole workspace 0xFF, bound (the bind zeroes the activations), members loaded, encode.  Then every byte the load left
    as it found it -- the packed batch, e0 / e1 / xe with their pad rows, the split-K slabs, the step buffers, noise and logits
    scratch, the counters -- is set to 0xFF (the set is taken from snapshots before and after the load, so no layout is restated; a
    byte the load wrote with the value it already had counts as not owned: re-poisoning it would break the run, loudly) and encode
    runs again, twice: the same bits as run 1 and as a handle whose workspace started as zeros.  So nd_encode needs no zeroed pad
    rows: it writes every row of every 16-row tile it reads."""
    H, F, K, B = ENC_DIMS[half]["H"], ENC_DIMS[half]["F"], 3, 17
    D = enc_data_dim(kind, half, K)
    members = enc_members(D, H, F, K, 80)
    x = rnd((B, D), 6).abs()
    zeros = enc_engine(D, H, F, K, 40, half, members, fill=0)
    encode(zeros, x)
    want = [read_stages(zeros, k, B) for k in range(K)]
    del zeros
    eng = enc_engine(D, H, F, K, 40, half, [], fill=0xFF)           # poisoned and bound, nothing loaded yet
    before = eng.workspace.clone()
    for k, p in enumerate(members):
        eng.load_member(k, p)
    torch.cuda.synchronize()
    not_owned = eng.workspace == before
    assert 0.02 < float(not_owned.float().mean()) < 0.98            # both kinds of bytes exist
    encode(eng, x)
    runs = [[read_stages(eng, k, B) for k in range(K)]]
    for _ in range(2):
        eng.workspace[not_owned] = 0xFF
        encode(eng, x)
        runs.append([read_stages(eng, k, B) for k in range(K)])
    for run in runs:
        for k in range(K):
            for a, b in zip(run[k], want[k]):
                assert bool(torch.isfinite(a).all()) and same_bits(a, b)


# ---- (d) the mapping MLP on the same stream ----------------------------------------------------------------------------------------
MLP_WIDTHS = (224, 96, 160)           # multiples of 32 (fp16 operands), none of 64
MLP_CLASSES = 3


def mlp_chain64(p, x, half):
    """Classifier.forward in float64 with the per-element bar carried through the four layers (ReLU is 1-Lipschitz; an fp16 handle
    rounds the three hidden activations to fp16: F16_ROUND of their magnitude joins the carried bar)."""
    h, hbar = operand64(x, half), torch.zeros_like(x, dtype=torch.float64)
    for l in range(1, 5):
        W, b = operand64(p[f"linear{l}.weight"].to(DEV), half), p[f"linear{l}.bias"].to(DEV).double()
        u = h @ W.T + b
        bar = (hbar @ W.abs().T) / GEMM_TOL + h.abs() @ W.abs().T + b.abs()        # incoming error + this layer's own rounding
        h, hbar = (torch.relu(u), bar * GEMM_TOL) if l < 4 else (u, bar * GEMM_TOL)
        if half and l < 4:                                           # (the reference keeps the unrounded value: one rounding, the kernel's)
            hbar = hbar + F16_ROUND * h.abs() + F16_SUBNORMAL
    return h, hbar / GEMM_TOL


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("B", [1, 17, 128, 129])
def test_classifier_chain(B, half):
    """Classifier.forward (four nd_linear calls): layer 1 split-K (in_features 16416), the last layer N = 3; B = 128 / 129 is the
    hand-over to the tiled form.  Logits against the float64 chain with the bar carried through the four layers."""
    from nested_diffusion_amd.mapping import Classifier
    D = 16416
    for l, (K_, N_) in enumerate(zip((D,) + MLP_WIDTHS, MLP_WIDTHS + (MLP_CLASSES,))):
        R = linear_route(K_, N_, B, half, ncu())
        assert_route_matches_library(R)
        assert R["route"] == ("splitk" if l == 0 else "tile" if B > 128 and not half else "stream")
    p = ref_cpu.init_classifier_params(D, widths=MLP_WIDTHS, num_classes=MLP_CLASSES, seed=31)
    x = rnd((B, D), 32)
    got = Classifier(p, dtype="f16" if half else "f32")(x)
    ref, bar = mlp_chain64(p, x, half)
    assert_close(got, ref, bar, f"classifier{'/fp16' if half else ''}: B={B}")


@pytest.mark.parametrize("dtype,B,K", [("f32", 17, 2), ("f32", 17, 8), ("f32", 17, 9), ("f16", 17, 8), ("f32", 129, 2), ("f16", 129, 2)])
def test_conditioner_mlp_tails(dtype, B, K, monkeypatch):
    """nd_guiding_prediction's mapping MLPs (nd_mlp_chain_first + nd_mlp_chain_tail, or nd_mlp_chain per member): layer 1 split-K
    (144 tokens x 128), K = 2 and 8 in the batched tail, K = 9 beyond it, B = 129 the tiled form with packed output.  Each member's
    logits against the float64 chain from the tokens its prefix block produced; the batched tail against the per-member sequence
    within the same per-element bar."""
    from nested_diffusion_amd.mapping import Classifier, GuidingConditioner, VisionTransformer
    half = dtype == "f16"
    heads, img, embed = 2, 192, 128
    vp = ref_cpu.init_vit_params(embed=embed, depth=K, patch=16, img=img, seed=3)
    vit = VisionTransformer(vp, heads, dtype=dtype)
    x = torch.rand(B, 3, img, img, generator=torch.Generator().manual_seed(15)).to(DEV)
    toks, tok = [], vit.patch_embed(x)
    for i in range(K):
        tok = vit.block(i, tok, B)
        toks.append(tok.reshape(B, -1).clone())
    D = toks[0].shape[1]
    assert D >= 16384
    mlps = [ref_cpu.init_classifier_params(D, widths=MLP_WIDTHS, num_classes=MLP_CLASSES, seed=20 + i) for i in range(K)]
    cond = GuidingConditioner(vit, [Classifier(m, dtype=dtype) for m in mlps])
    monkeypatch.delenv("ND_MLP_TAIL_PER_MEMBER", raising=False)
    shared = cond.compute_guiding_prediction(x, include_full_vit=False)
    monkeypatch.setenv("ND_MLP_TAIL_PER_MEMBER", "1")
    single = cond.compute_guiding_prediction(x, include_full_vit=False)
    monkeypatch.delenv("ND_MLP_TAIL_PER_MEMBER")
    for k in range(K):
        ref, bar = mlp_chain64(mlps[k], toks[k], half)
        assert_close(single[k], ref, bar, f"mlp per member/{dtype}: B={B} K={K} member {k}")
        assert_close(shared[k], ref, bar, f"mlp batched tail/{dtype}: B={B} K={K} member {k}")
        if K > 8 or (B > 128 and not half):
            assert torch.equal(shared[k], single[k])                  # no batched form for this shape: the same launches


@pytest.fixture(scope="module", autouse=True)
def report_worst_normalised_errors():
    """prints the worst per-element normalised error of each stage over the module (the bars are asserted per check)."""
    yield
    for key, err in sorted(WORST.items()):
        print(f"\nworst normalised error {key:28s} {err:.3e}", end="")
    for key, (e_k, e_t) in sorted(FP32_RULE.items()):
        print(f"\nfp32-relative rule {key:32s} kernel {e_k:.3f} ulp, torch fp32 {e_t:.3f} ulp, ratio {e_k / max(e_t, 1e-300):.2f}", end="")
