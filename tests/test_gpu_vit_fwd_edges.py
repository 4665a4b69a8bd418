"""Edge shapes and launch-plan coverage of the ViT forward kernels: the fp32 GEMM on the bf16 pipe (nd_gemm_split, csrc/nd_gemm_b9.hip)
and the f32-MFMA / fp16 GEMM (nd_gemm_bias_act, csrc/nd_gemm_nt.hip) at every branch of their tile plans, the qkv-image GEMM, the three
attention forms, LayerNorm in both output forms and patchify.

The two tile plans are restated here (`b9_plan`, `gemm_plan`) with the device's CU count; every shape the tests use is cross-checked
against the library's workspace sizes, and shapes are found by searching a small grid for each branch, so that a device whose CU count
moves the branches makes the search (and the test) fail loudly instead of covering less.

References: float64 on the same fp32 inputs (the fp16 forms: on fp16-rounded operands, as tests/test_gpu_fp16.py), computed on the GPU.
Bars are per element: a GEMM element's error is divided by (|x| @ |w|^T)_ij + |bias_j| + |residual_ij|, an attention element's by
(P @ |v|)_ij, so one wrong row, column or tile fails.  In the ill-conditioned regimes (peaked or huge scores, far-off-centre or outlier
LayerNorm rows) the kernel must stay within 4x of torch's own fp32 against float64 (`within_fp32`).  Exact paths are compared bit for
bit.  Outputs and split-K workspaces are buffers of 0xFF bytes before each call, so an element or slab nobody wrote reads as NaN."""
import functools

import pytest
import torch
import torch.nn.functional as F

from test_gpu_grad_edges import assert_image_is_split_of, check, image_buffer, image_pieces, lib, p, poisoned, stream, within_fp32

pytestmark = pytest.mark.gpu
DEV = "cuda"
LN_EPS = 1e-6
GEMM_TOL = 1e-5                  # per-element normalised error of an fp32-accumulated GEMM (measured <= ~1e-6)
ATT_TOL = 1e-5                   # per-element normalised error of the attention on well-conditioned (randn) inputs
F16_ATT_TOL = 5e-4               # the fp16 attention bar of tests/test_gpu_fp16.py (of max(1, |ref|max))
ACT_NONE, ACT_GELU = 0, 3
F32, F16 = 0, 1


@functools.lru_cache(None)
def ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- the two GEMM tile plans, restated ------------------------------------------------------------------------------------------
def b9_plan(M, K, N):
    """nd_b9_plan (csrc/nd_gemm_b9.hip): (branch, split, workspace bytes).  K >= 2048: 'wide' 128 x 128 tiles, one workgroup per CU,
    a partly filled last round cut into k-slabs s in {2, 3, 4, 6, 8} by a cost model; else 64 x 128 tiles, two per CU, a small
    remainder sent out as half tiles (split = -1)."""
    wide = K >= 2048
    BM, BN = (128 if wide else 64), 128
    tiles = -(-M // BM) * -(-N // BN)
    slots = ncu() * (1 if wide else 2)
    rem, nkb, split = tiles % slots, K // 32, 1
    if rem > 0 and tiles > slots and not wide:
        split = -1 if 2 * rem <= ncu() else 1
    elif rem > 0 and tiles > slots:
        best = nkb * 1.4 + 4.0
        for s in (2, 3, 4, 6, 8):
            if nkb // s < 4:
                continue
            slabs = rem * s
            t = ((slabs + slots - 1) // slots) * (nkb / s * 1.4 + 5.0) + 5.0 + slabs * BM * BN * 4.0 * 2.0 / 3.0e6
            if t < best - 1e-9:
                best, split = t, s
    if tiles <= slots or rem == 0:
        branch = "wide_fits" if wide else "narrow_fits"
    elif wide:
        branch = f"wide_split{split}" if split > 1 else "wide_whole_tail"
    else:
        branch = "narrow_half_tail" if split == -1 else "narrow_whole_tail"
    return branch, split, (rem * split * BM * BN * 4 if split > 1 else 0)


def gemm_plan(M, K, N, dtype):
    """nd_gemm_plan (csrc/nd_gemm_nt.hip): (split, workspace bytes).  128 x 64 tiles, one per CU per round; when M N K >= 2^28 the
    tiles % CUs remainder is cut into s in {1, .., 6, 8} k-slabs, the smallest s within 10 % of the shortest tail."""
    bk = 32 if dtype == F16 else 16
    tiles = -(-M // 128) * -(-N // 64)
    rem, nk, split = tiles % ncu(), K // bk, 1
    if rem > 0 and M * N * K >= 1 << 28:
        cand = [s for s in (1, 2, 3, 4, 5, 6, 8) if nk // s >= 8]
        best = min(((rem * s + ncu() - 1) // ncu()) / s for s in cand)
        split = next(s for s in cand if ((rem * s + ncu() - 1) // ncu()) / s <= best * 1.1 + 1e-9)
    return split, (rem * split * 128 * 64 * 4 if split > 1 else 0)


def qkv_plan(B, ntok, heads):
    """the plan of nd_gemm_split_qkv: the two-per-CU shape, whole tiles or a half-tile tail, never k-slabs."""
    tiles, slots = -(-(B * ntok) // 64) * (3 * heads * 64 // 128), 2 * ncu()
    rem = tiles % slots
    if rem == 0 or tiles <= slots:
        return "fits"
    return "half_tail" if 2 * rem <= ncu() else "whole_tail"


KINDS = {"aligned": ("aligned", "aligned"), "ragged_m": ("ragged", "aligned"), "ragged_n": ("aligned", "ragged")}


def find_shape(plan_branch, want, kind, Ks, m_unit, n_unit, n_ragged):
    """the cheapest (M N K) of a small grid, of the given kind, whose restated plan takes `want`.  ragged M: M % m_unit != 0 and
    M % 16 != 0; ragged N: N % n_unit = n_unit - n_ragged."""
    mk, nk = KINDS[kind]
    Ms = [m_unit * k - (56 if mk == "ragged" else 0) for k in range(1, 65)]
    Ns = [n_unit * j - (n_ragged if nk == "ragged" else 0) for j in range(1, 97)]
    for _, M, K, N in sorted((M * K * N, M, K, N) for M in Ms for N in Ns for K in Ks):
        if plan_branch(M, K, N) == want:
            return M, K, N
    raise AssertionError(f"no {kind} shape in the grid reaches {want} on {ncu()} CUs")


B9_BRANCHES = ["narrow_fits", "narrow_half_tail", "narrow_whole_tail", "wide_fits", "wide_whole_tail",
               "wide_split2", "wide_split3", "wide_split4", "wide_split6", "wide_split8"]


def b9_shape(branch, kind):
    Ks = (2048, 3072, 4096, 6144) if branch.startswith("wide") else (768, 1024)
    return find_shape(lambda M, K, N: b9_plan(M, K, N)[0], branch, kind, Ks, 128, 128, 32)


def bias_act_shape(split, dtype, kind):
    def branch(M, K, N):
        if (-(-M // 128) * -(-N // 64)) % ncu() == 0:       # no remainder: not the tail this case is after
            return None
        return gemm_plan(M, K, N, dtype)[0]
    return find_shape(branch, split, kind, (256, 512, 768, 1024, 2048, 3072), 128, 64, 30)


# ---- inputs, references, bars ------------------------------------------------------------------------------------------------------
def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def gemm_inputs(M, K, N, seed, row_sigma=4.0):
    """x with row scales exp(row_sigma * randn), w ~ randn / sqrt(K), bias and residual at the scale of the output."""
    g = gen(seed)
    x = torch.randn(M, K, generator=g, device=DEV) * torch.exp(row_sigma * torch.randn(M, 1, generator=g, device=DEV))
    w = torch.randn(N, K, generator=g, device=DEV) / K ** 0.5
    b = torch.randn(N, generator=g, device=DEV)
    r = torch.randn(M, N, generator=g, device=DEV) * x.abs().mean(1, keepdim=True)
    return x, w, b, r


def gemm_ref(x, w, b, r, act):
    """float64 act(x w^T + b) + r and the per-element scale (|x| @ |w|^T + |b|) * 1.2 + |r| (1.2 >= max |GELU'|)."""
    xd, wd = x.double(), w.double()
    t = xd @ wd.T
    scale = xd.abs() @ wd.abs().T
    if b is not None:
        t += b.double()
        scale += b.double().abs()
    if act == ACT_GELU:
        t, scale = F.gelu(t), 1.2 * scale
    if r is not None:
        t += r.double()
        scale += r.double().abs()
    return t, scale


def assert_per_element(out, ref, scale, tol, what):
    err = (out.double() - ref).abs() / scale.clamp_min(1e-300)
    bad = ~(err <= tol)                                                            # NaN counts as bad
    if bool(bad.any()):
        i, j = (int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements off the bar {tol:g}, first at ({i}, {j}): "
                             f"got {float(out[i, j])}, want {float(ref[i, j])}; rows hit {bad.any(1).nonzero().flatten()[:8].tolist()}, "
                             f"columns hit {bad.any(0).nonzero().flatten()[:8].tolist()}")
    return float(err.max())


def poison_pad_rows(img):
    """a copy of a frag32b3 image whose pad rows (rows .. 16 * ceil(rows / 16) - 1 of the last block row) are 0xFF bytes."""
    out = image_buffer(img.rows, img.K, 0)
    out.data.copy_(img.data)
    nkb, r0 = img.K // 32, img.rows % 16
    if r0:
        last = out.data[((img.rows // 16) * nkb) * 3072: ((img.rows // 16) + 1) * nkb * 3072].view(torch.int16)
        last.view(nkb, 3, 4, 16, 8)[:, :, :, r0:, :] = -1
        assert bool((image_pieces(out, pad=True)[img.rows:] == -1).all())
    return out


def gemm_split_abi(xs, ws, b, r, M, K, N, act, workspace=True, want_split=True):
    """nd_gemm_split through the C ABI into poisoned outputs and a poisoned workspace of the plan's size."""
    nbytes = lib().nd_gemm_split_workspace_bytes(M, K, N) if workspace else 0
    wsp = torch.full((max(nbytes, 16),), 0xFF, dtype=torch.uint8, device=DEV) if nbytes else None
    out = poisoned(M, N)
    osp = image_buffer(M, N) if want_split and N % 32 == 0 else None
    check(lib().nd_gemm_split(p(xs.data), p(ws.data), p(b), p(r), p(out), p(osp.data) if osp else None, M, K, N, act, p(wsp), nbytes,
                              stream()), "nd_gemm_split")
    return out, osp


def run_gemm_split_case(M, K, N, seed, scales=(-20, 20)):
    """every option of nd_gemm_split at one shape: residual / none, act none / gelu, the fp32 output and the frag32b3 image, workspace /
    none, run-to-run reproducibility, pad rows of the operand images poisoned, global input scales 2^s."""
    from nested_diffusion_amd import ops
    branch, split, ws_bytes = b9_plan(M, K, N)
    assert lib().nd_gemm_split_workspace_bytes(M, K, N) == ws_bytes, (M, K, N, branch, "the restated plan disagrees with the library")
    x, w, b, r = gemm_inputs(M, K, N, seed)
    xs, wsm = ops.split_rows(x), ops.split_rows(w)
    what = f"gemm_split M={M} K={K} N={N} ({branch})"
    ref, scale = gemm_ref(x, w, b, r, ACT_NONE)
    out, osp = gemm_split_abi(xs, wsm, b, r, M, K, N, ACT_NONE)
    err1 = assert_per_element(out, ref, scale, GEMM_TOL, what + " residual, act none")
    if osp is not None:
        assert_image_is_split_of(osp, out)
    again, _ = gemm_split_abi(xs, wsm, b, r, M, K, N, ACT_NONE, want_split=False)
    assert torch.equal(again, out), what + ": not reproducible (fp32 output alone)"
    whole, _ = gemm_split_abi(xs, wsm, b, r, M, K, N, ACT_NONE, workspace=False)
    assert_per_element(whole, ref, scale, GEMM_TOL, what + " without workspace")
    assert torch.equal(gemm_split_abi(xs, wsm, b, r, M, K, N, ACT_NONE, workspace=False)[0], whole), what + ": not reproducible, no workspace"
    if split <= 1:
        assert torch.equal(whole, out), what + ": no k-split, yet the workspace changed the result"
    refg, scaleg = gemm_ref(x, w, b, None, ACT_GELU)
    outg, ospg = gemm_split_abi(xs, wsm, b, None, M, K, N, ACT_GELU)
    assert_per_element(outg, refg, scaleg, GEMM_TOL, what + " gelu, no residual")
    if ospg is not None:
        assert_image_is_split_of(ospg, outg)
    if M % 16 or N % 16:
        pout, _ = gemm_split_abi(poison_pad_rows(xs), poison_pad_rows(wsm), b, r, M, K, N, ACT_NONE, want_split=False)
        assert torch.equal(pout, out), what + ": poisoned pad rows of the operand images reached the result"
    for s in scales:
        f = 2.0 ** s
        sx = ops.split_rows(x * f)
        got, _ = gemm_split_abi(sx, wsm, b * f, r * f, M, K, N, ACT_NONE, want_split=False)
        err = assert_per_element(got, ref * f, scale * f, GEMM_TOL, what + f" inputs x 2^{s}")
        assert err <= 2 * err1 + 2 ** -23, (what, s, err, err1)           # the normalised error does not depend on the scale
    return branch


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("branch", B9_BRANCHES)
def test_gemm_split_plan_branch(branch, kind, record_property):
    """Each branch of nd_b9_plan, reached on this device (the restated plan and the workspace size agree): narrow (K < 2048) whole
    tiles / half-tile tail / whole tail, wide whole tiles / whole tail / k-split s = 2, 3, 4, 6, 8 with k_b9_fixup; each with a ragged
    last row tile, a ragged last column tile, and both aligned."""
    M, K, N = b9_shape(branch, kind)
    record_property("shape", f"{M}x{K}x{N}")
    print(f"{branch} {kind}: M={M} K={K} N={N}")
    assert run_gemm_split_case(M, K, N, seed=M + K + N) == branch


@pytest.mark.parametrize("M", [6304, 6272])
@pytest.mark.parametrize("K,N", [(768, 2304), (768, 768), (768, 3072), (3072, 768)])
def test_gemm_split_production_shapes(M, K, N, record_property):
    """The four Linear layers of ViT-B/16 (qkv, proj, fc1, fc2) at B = 32 x 197 and 32 x 196 tokens."""
    record_property("branch", b9_plan(M, K, N)[0])
    run_gemm_split_case(M, K, N, seed=M + 7 * N, scales=())


# ---- nd_gemm_bias_act (f32 MFMA and fp16 operands) ---------------------------------------------------------------------------------
def bias_act_abi(x, w, b, r, M, K, N, act, dtype, workspace=True):
    nbytes = lib().nd_gemm_workspace_bytes(M, K, N, dtype) if workspace else 0
    wsp = torch.full((max(nbytes, 16),), 0xFF, dtype=torch.uint8, device=DEV) if nbytes else None
    out = poisoned(M, N)
    check(lib().nd_gemm_bias_act(p(x), p(w), p(b), p(r), p(out), M, K, N, act, dtype, p(wsp), nbytes, stream()), "nd_gemm_bias_act")
    return out


def run_bias_act_case(M, K, N, dtype, seed):
    split, ws_bytes = gemm_plan(M, K, N, dtype)
    assert lib().nd_gemm_workspace_bytes(M, K, N, dtype) == ws_bytes, (M, K, N, dtype, "the restated plan disagrees with the library")
    # fp16 operands: rows kept inside fp16's normal range (exp(4 randn) row scales would overflow 65504 or go subnormal)
    x, w, b, r = gemm_inputs(M, K, N, seed, row_sigma=4.0 if dtype == F32 else 0.5)
    wk = w.half() if dtype == F16 else w
    xr, wr = (x.half().float(), w.half().float()) if dtype == F16 else (x, w)
    what = f"gemm_bias_act {'f16' if dtype else 'f32'} M={M} K={K} N={N} split={split}"
    ref, scale = gemm_ref(xr, wr, b, r, ACT_NONE)
    out = bias_act_abi(x, wk, b, r, M, K, N, ACT_NONE, dtype)
    assert_per_element(out, ref, scale, GEMM_TOL, what + " residual, act none")
    assert torch.equal(bias_act_abi(x, wk, b, r, M, K, N, ACT_NONE, dtype), out), what + ": not reproducible"
    whole = bias_act_abi(x, wk, b, r, M, K, N, ACT_NONE, dtype, workspace=False)
    assert_per_element(whole, ref, scale, GEMM_TOL, what + " without workspace")
    assert torch.equal(bias_act_abi(x, wk, b, r, M, K, N, ACT_NONE, dtype, workspace=False), whole), what + ": not reproducible, no workspace"
    refg, scaleg = gemm_ref(xr, wr, b, None, ACT_GELU)
    assert_per_element(bias_act_abi(x, wk, b, None, M, K, N, ACT_GELU, dtype), refg, scaleg, GEMM_TOL, what + " gelu, no residual")
    if dtype == F32:
        for s in (-20, 20):
            f = 2.0 ** s
            got = bias_act_abi(x * f, wk, b * f, r * f, M, K, N, ACT_NONE, dtype)
            assert_per_element(got, ref * f, scale * f, GEMM_TOL, what + f" inputs x 2^{s}")
    return split


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("split", [1, 2, 3, 4, 5, 6, 8])
@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_gemm_bias_act_plan_split(dtype, split, kind, record_property):
    """Each k-split s of nd_gemm_plan (s = 1: a partly filled last round left whole) with k_gemm_fixup, in the f32-MFMA kernel and the
    fp16-operand kernel; ragged last row tile, ragged last column tile (N % 4 != 0: the scalar store), both aligned."""
    M, K, N = bias_act_shape(split, dtype, kind)
    record_property("shape", f"{M}x{K}x{N}")
    print(f"{'f16' if dtype else 'f32'} s={split} {kind}: M={M} K={K} N={N}")
    assert run_bias_act_case(M, K, N, dtype, seed=M + K + N + dtype) == split


@pytest.mark.parametrize("M", [6304, 6272])
@pytest.mark.parametrize("K,N", [(768, 2304), (768, 768), (768, 3072), (3072, 768)])
def test_gemm_fp16_production_shapes(M, K, N):
    """The fp16 mode's Linear layers at the conditioner's token counts (s = 2 and 3 of its plan)."""
    run_bias_act_case(M, K, N, F16, seed=M + 5 * N)


# ---- attention ---------------------------------------------------------------------------------------------------------------------
ATT_KINDS = ["randn", "peaked", "dominant", "constant", "huge"]


def attention_qkv(N, heads, seed, kinds=ATT_KINDS):
    """[len(kinds) * N, 3 * heads * 64]: image b carries inputs of kind kinds[b].
    randn: q, k, v ~ N(0, 1).  peaked: q, k x 2.5, scores spread ~20-40 over a row.  dominant: one key per head (the last key for
    head 0) leads every query's scores by ~100, the other weights underflow.  constant: q = 0, every score 0, the output is the mean
    of v.  huge: every score in 116..124 with no leader: exp without the max subtraction overflows fp32."""
    g = gen(seed)
    E = heads * 64
    t = torch.randn(len(kinds), N, 3, heads, 64, generator=g, device=DEV)
    for b, kind in enumerate(kinds):
        q, k = t[b, :, 0], t[b, :, 1]
        if kind == "peaked":
            q *= 2.5
            k *= 2.5
        elif kind == "dominant":
            q.mul_(0.01)[..., 0] = 10.0
            k.mul_(0.01)
            for h in range(heads):
                k[(N - 1 if h == 0 else (7 * h + 3) % N), h, 0] = 80.0             # score 10 * 80 / 8 = 100
        elif kind == "constant":
            q.zero_()
        elif kind == "huge":
            q.mul_(0.001)[..., 0] = 30.0
            k.mul_(0.001)[..., 0] = 32.0 * (1 + 0.03 * torch.rand(N, heads, generator=g, device=DEV))
    return t.reshape(len(kinds) * N, 3 * E)


def attention_ref(qkv, B, N, heads, dtype=torch.float64):
    """softmax(q k^T / 8) v in `dtype`, and the per-element scale P @ |v| (float64)."""
    t = qkv.to(dtype).reshape(B, N, 3, heads, 64).permute(2, 0, 3, 1, 4)
    a = ((t[0] @ t[1].transpose(-2, -1)) * 0.125).softmax(-1)
    o = (a @ t[2]).transpose(1, 2).reshape(B * N, heads * 64)
    return o, (a.double() @ t[2].double().abs()).transpose(1, 2).reshape(B * N, heads * 64)


def check_attention_kinds(out, qkv, N, heads, kinds, what):
    """randn and constant images at ATT_TOL per element; the others by the fp32-relative rule on their worst normalised element."""
    B = len(kinds)
    assert bool(torch.isfinite(out).all()), what + ": non-finite output"
    ref, scale = attention_ref(qkv, B, N, heads)
    ref32, _ = attention_ref(qkv, B, N, heads, torch.float32)
    err = ((out.double() - ref).abs() / scale).reshape(B, N, -1)
    err32 = ((ref32.double() - ref).abs() / scale).reshape(B, N, -1)
    for b, kind in enumerate(kinds):
        e, e32 = float(err[b].max()), float(err32[b].max())
        if kind in ("randn", "constant"):
            assert e <= ATT_TOL, (what, kind, e)
        else:
            assert within_fp32(e, e32, ATT_TOL), (what, kind, e, e32)


def attention_abi(qkv, B, N, heads, dtype=F32):
    out = poisoned(B * N, heads * 64)
    check(lib().nd_attention(p(qkv), p(out), B, N, heads, 64, dtype, stream()), "nd_attention")
    return out


def attention_split_abi(qkv, B, N, heads):
    img = image_buffer(B * N, heads * 64)
    check(lib().nd_attention_split(p(qkv), p(img.data), B, N, heads, 64, stream()), "nd_attention_split")
    return img


@pytest.mark.parametrize("heads", [1, 3, 12, 16])
def test_attention_f32_every_n(heads):
    """k_attention_ring (nd_attention, nd_attention_split) at every N from 1 to 256: all 16 NF instantiations, every NT choice, every
    clamp of the last fragment; the five input kinds of attention_qkv as five images of one call."""
    for N in range(1, 257):
        what = f"nd_attention N={N} heads={heads}"
        qkv = attention_qkv(N, heads, seed=N * 100 + heads)
        B = len(ATT_KINDS)
        out = attention_abi(qkv, B, N, heads)
        check_attention_kinds(out, qkv, N, heads, ATT_KINDS, what)
        assert torch.equal(attention_abi(qkv, B, N, heads), out), what + ": not reproducible"
        assert_image_is_split_of(attention_split_abi(qkv, B, N, heads), out)


def test_attention_f32_conditioner_batch():
    """B = 32 x 197 tokens x 12 heads (4608 workgroups), randn inputs, and the split image of the same call."""
    B, N, heads = 32, 197, 12
    qkv = attention_qkv(N, heads, seed=197, kinds=["randn"] * B)
    out = attention_abi(qkv, B, N, heads)
    check_attention_kinds(out, qkv, N, heads, ["randn"] * B, "nd_attention B=32 N=197")
    assert torch.equal(attention_abi(qkv, B, N, heads), out)
    assert_image_is_split_of(attention_split_abi(qkv, B, N, heads), out)


@pytest.mark.parametrize("heads", [2, 4, 12, 16])
def test_attention_images_every_n(heads):
    """k_attention_b9 from the qkv images at every supported N (4 .. 256, step 4): every njw body.  The qkv GEMM runs with an identity
    weight, so the images hold the chosen q, k, v exactly and all five input kinds reach the attention."""
    from nested_diffusion_amd import ops
    E3 = 3 * heads * 64
    eye = ops.split_rows(torch.eye(E3, device=DEV))
    B = len(ATT_KINDS)
    for N in range(4, 257, 4):
        what = f"nd_attention_images N={N} heads={heads}"
        qkv = attention_qkv(N, heads, seed=N * 100 + heads + 7)
        nbytes = lib().nd_qkv_images_bytes(B, N, heads)
        buf = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
        img = ops.gemm_split_qkv(ops.split_rows(qkv), eye, None, B, N, heads, out=buf)
        out = poisoned(B * N, heads * 64)
        check(lib().nd_attention_images(p(img), p(out), 0, B, N, heads, stream()), "nd_attention_images")
        check_attention_kinds(out, qkv, N, heads, ATT_KINDS, what)
        again = poisoned(B * N, heads * 64)
        check(lib().nd_attention_images(p(img), p(again), 0, B, N, heads, stream()), "nd_attention_images")
        assert torch.equal(again, out), what + ": not reproducible"
        sp = image_buffer(B * N, heads * 64)
        check(lib().nd_attention_images(p(img), p(sp.data), 1, B, N, heads, stream()), "nd_attention_images")
        assert_image_is_split_of(sp, out)


@pytest.mark.parametrize("tail", ["half_tail", "whole_tail"])
def test_gemm_split_qkv_tails(tail, record_property):
    """nd_gemm_split_qkv's half-tile tail and whole tail (B chosen from the restated plan, 196 tokens, 12 heads, K = 768), checked
    through nd_attention_images against float64 of the whole qkv Linear + attention."""
    from nested_diffusion_amd import ops
    N, heads, K = 196, 12, 768
    B = next(b for b in range(1, 129) if qkv_plan(b, N, heads) == tail)
    record_property("B", B)
    E = heads * 64
    g = gen(B)
    x = torch.randn(B * N, K, generator=g, device=DEV)
    w = torch.randn(3 * E, K, generator=g, device=DEV) / K ** 0.5
    bias = torch.randn(3 * E, generator=g, device=DEV) * 0.1
    buf = torch.full((lib().nd_qkv_images_bytes(B, N, heads),), 0xFF, dtype=torch.uint8, device=DEV)
    img = ops.gemm_split_qkv(ops.split_rows(x), ops.split_rows(w), bias, B, N, heads, out=buf)
    out = ops.attention_images(img, B, N, heads)
    qkv64 = x.double() @ w.double().T + bias.double()
    ref, scale = attention_ref(qkv64, B, N, heads)
    assert bool(torch.isfinite(out).all())
    assert_per_element(out, ref, scale, ATT_TOL, f"qkv images {tail} B={B}")


@pytest.mark.parametrize("heads", [1, 12])
def test_attention_f16_every_n(heads):
    """k_attention_h (nd_attention dtype f16) at every N from 1 to 256 and the five input kinds, against torch on fp16-rounded q, k, v
    and fp16-rounded probabilities (fp32 softmax and sums).  randn, dominant and constant images at the bar of tests/test_gpu_fp16.py
    (5e-4 of max(1, |ref|max)).  Peaked and huge scores put probabilities near 1, where the kernel's and torch's fp32 softmax, an ulp
    apart, can round to neighbouring fp16 values 2^-11 apart (measured: 1.92e-3 against a bar of 1.83e-3 at N = 132): there the bar is
    per element, two fp16 steps of the probabilities, 2^-10 (P @ |v|)."""
    B = len(ATT_KINDS)
    for N in range(1, 257):
        qkv = attention_qkv(N, heads, seed=N * 10 + heads + 3)
        out = attention_abi(qkv, B, N, heads, F16)
        assert bool(torch.isfinite(out).all()), (N, heads)
        t = qkv.half().double().reshape(B, N, 3, heads, 64).permute(2, 0, 3, 1, 4)
        a = ((t[0] @ t[1].transpose(-2, -1)) * 0.125).float().softmax(-1)
        ref = (a.half().double() @ t[2]).transpose(1, 2).reshape(B, N * heads * 64)
        scale = (a.double() @ t[2].abs()).transpose(1, 2).reshape(B, N * heads * 64)
        diff = (out.double().reshape(B, -1) - ref).abs()
        for b, kind in enumerate(ATT_KINDS):
            if kind in ("peaked", "huge"):
                assert bool((diff[b] <= 2.0 ** -10 * scale[b]).all()), (N, heads, kind, float((diff[b] / scale[b]).max()))
            else:
                bound = F16_ATT_TOL * max(1.0, float(ref[b].abs().max()))
                assert float(diff[b].max()) <= bound, (N, heads, kind, float(diff[b].max()), bound)
        assert torch.equal(attention_abi(qkv, B, N, heads, F16), out), (N, heads)


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------
LN_ROW_KINDS = ["random", "off_centre", "constant", "outlier"]


def layernorm_inputs(rows, dim, seed):
    """row i is of kind LN_ROW_KINDS[i % 4]: randn * 2 + 0.3; mean 1e4 and std 1e-2; constant 0.7; randn with one entry 100x the rest."""
    g = gen(seed)
    x = torch.randn(rows, dim, generator=g, device=DEV) * 2 + 0.3
    kind = [LN_ROW_KINDS[i % 4] for i in range(rows)]
    for i, k in enumerate(kind):
        if k == "off_centre":
            x[i] = 1e4 + 1e-2 * torch.randn(dim, generator=g, device=DEV)
        elif k == "constant":
            x[i] = 0.7
        elif k == "outlier":
            x[i, (7 * i) % dim] = 100 * float(x[i].abs().max())
    w = 1 + 0.1 * torch.randn(dim, generator=g, device=DEV)
    b = 0.1 * torch.randn(dim, generator=g, device=DEV)
    return x, w, b, kind


def layernorm_abi(x, w, b):
    rows, dim = x.shape
    out = poisoned(rows, dim)
    check(lib().nd_layernorm(p(x), p(w), p(b), p(out), rows, dim, LN_EPS, stream()), "nd_layernorm")
    return out


def layernorm_split_abi(x, w, b):
    rows, dim = x.shape
    img = image_buffer(rows, dim)
    check(lib().nd_layernorm_split(p(x), p(w), p(b), p(img.data), rows, dim, LN_EPS, stream()), "nd_layernorm_split")
    return img


def check_layernorm(out, x, w, b, kind, what):
    """per element: error against float64 over |gamma| (|xhat| + 1) + |beta| (an error in the row's mean moves every element by
    |gamma| times it over the spread: |gamma * xhat| + |beta| alone is near 0 for some of a million elements); the worst element of
    each row kind by the fp32-relative rule against torch's F.layer_norm in fp32 (floor 1e-5); constant rows give beta within 4 ulps."""
    dim = x.shape[1]
    ref = F.layer_norm(x.double(), (dim,), w.double(), b.double(), LN_EPS)
    t32 = F.layer_norm(x, (dim,), w, b, LN_EPS).double()
    xh = F.layer_norm(x.double(), (dim,), None, None, LN_EPS)
    scale = w.double().abs() * (xh.abs() + 1) + b.double().abs()
    err = ((out.double() - ref).abs() / scale).amax(1).cpu()
    err32 = ((t32 - ref).abs() / scale).amax(1).cpu()
    assert bool(torch.isfinite(out).all()), what + ": non-finite output"
    for k in LN_ROW_KINDS:
        rows = [i for i, kk in enumerate(kind) if kk == k]
        if not rows:
            continue
        e, e32 = float(err[rows].max()), float(err32[rows].max())
        print(f"{what} {k}: kernel {e:.3e}, torch fp32 {e32:.3e}")
        assert within_fp32(e, e32, 1e-5), (what, k, e, e32)
        if k == "constant":
            ulp = torch.finfo(torch.float32).eps * b.abs()
            d = float(((out[rows] - b).abs() / ulp).max())
            assert d <= 4, (what, "constant rows are not beta", d)


LN_DIMS = [4, 36, 100, 252, 256, 260, 508, 512, 516, 764, 768, 1000, 1024, 1028, 1536, 2044, 2048]


@pytest.mark.parametrize("dim", LN_DIMS)
def test_layernorm_sweep(dim):
    """k_layernorm<1, 2, 3, 4, 8>: the dims on either side of every VPL boundary, dims that are no multiple of 64 (or of 32); rows
    off the 4-rows-per-workgroup grid; random, off-centre, constant and outlier rows."""
    for rows in (1, 3, 4, 5, 17, 591):
        x, w, b, kind = layernorm_inputs(rows, dim, seed=rows * 10000 + dim)
        out = layernorm_abi(x, w, b)
        check_layernorm(out, x, w, b, kind, f"nd_layernorm rows={rows} dim={dim}")
        assert torch.equal(layernorm_abi(x, w, b), out)


@pytest.mark.parametrize("dim", [32, 288, 512, 544, 800, 1024, 1056, 2048])
def test_layernorm_split_forms(dim):
    """nd_layernorm_split is nd_layernorm's output bit for bit: the direct form (rows < 64, or dim > 1024) and k_layernorm_split16
    at every VPL (rows >= 64, dim <= 1024), rows 64, 65, 79 (the first partial 16-row block), 80 and 6304."""
    for rows in (1, 17, 63, 64, 65, 79, 80, 6304):
        x, w, b, kind = layernorm_inputs(rows, dim, seed=rows * 1000 + dim)
        out = layernorm_abi(x, w, b)
        check_layernorm(out, x, w, b, kind, f"nd_layernorm rows={rows} dim={dim}")
        assert_image_is_split_of(layernorm_split_abi(x, w, b), out)


# ---- patchify ----------------------------------------------------------------------------------------------------------------------
def unfold_cols(img, patch):
    B, Cin, H, W = img.shape
    return F.unfold(img, patch, stride=patch).transpose(1, 2).reshape(B * (H // patch) * (W // patch), Cin * patch * patch)


PATCH_CASES = [(B, Cin, H, W, patch) for patch, H, W in ((4, 32, 48), (8, 40, 64), (12, 36, 60), (16, 48, 80), (28, 56, 84), (32, 64, 96))
               for Cin in (1, 2, 3) for B in (1, 3)] + [(32, 3, 224, 224, 16), (32, 3, 224, 224, 32), (32, 3, 224, 224, 28),
                                                        (32, 3, 224, 224, 8), (32, 2, 216, 216, 12)]


def test_patchify_is_unfold():
    """nd_patchify bit for bit = F.unfold; nd_patchify_split = the split of that (the gather form when p % 8 == 0, the element-wise form
    otherwise) wherever Cin p^2 % 32 == 0; every accepted p, one to three channels, non-square images, B = 32 at 224^2."""
    split_forms = set()
    for B, Cin, H, W, patch in PATCH_CASES:
        img = torch.randn(B, Cin, H, W, generator=gen(B * 100 + Cin * 10 + patch), device=DEV)
        R, C = B * (H // patch) * (W // patch), Cin * patch * patch
        cols = poisoned(R, C)
        check(lib().nd_patchify(p(img), p(cols), B, Cin, H, W, patch, stream()), "nd_patchify")
        assert torch.equal(cols, unfold_cols(img, patch)), (B, Cin, H, W, patch)
        if C % 32 == 0:
            sp = image_buffer(R, C)
            check(lib().nd_patchify_split(p(img), p(sp.data), B, Cin, H, W, patch, stream()), "nd_patchify_split")
            assert_image_is_split_of(sp, cols)
            split_forms.add("gather" if patch % 8 == 0 else "elementwise")
    assert split_forms == {"gather", "elementwise"}


def test_patchify_rejects_bad_shapes():
    """p = 14 (no multiple of 4), p not dividing the image, a split output with Cin p^2 % 32 != 0: an error, nothing launched."""
    img = torch.zeros(1, 3, 224, 224, device=DEV)
    cols = torch.zeros(1 << 20, device=DEV)
    assert lib().nd_patchify(p(img), p(cols), 1, 3, 224, 224, 14, stream()) != 0
    assert lib().nd_patchify(p(img), p(cols), 1, 3, 224, 224, 12, stream()) != 0          # 224 % 12 != 0
    assert lib().nd_patchify_split(p(img), p(cols), 1, 3, 224, 224, 14, stream()) != 0
    assert lib().nd_patchify_split(p(img), p(cols), 1, 1, 224, 224, 4, stream()) != 0     # 1 * 4^2 = 16
    assert torch.equal(cols, torch.zeros_like(cols))
