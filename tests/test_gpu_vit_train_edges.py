"""Edge shapes and dispatch coverage of the ViT training kernels (csrc/nd_vit_train.hip: nd_gemm_tn_adamw, nd_colsum_adamw,
nd_layernorm_wgrad_adamw) and of ViTTrainer at batches that cross a chunk of rows.

Which case launches which kernel form:
- k_gemm_tn_adamw<false> (gradient only): the M sweep of section 1 on both sides of every step of four rows and stage of 32 (grid 1 x 1),
  the 3 x 3 grid of section 2, and every reference gradient of section 3 (grid_n = 2).
- k_gemm_tn_adamw<true> (fused): section 3 on 'ragged' (2 x 2 tiles, ragged both ways) and (64, 65, 64) (grid_n = 2, one live row in the
  second N tile), with and without g_out, every written buffer inside guard zones; section 5 at (15, 17, 48).
- k_colsum_adamw<64, 16> (M <= 128): section 4 at M = 2 over N = 1 .. 151296 (1 .. 2364 workgroups), section 5 at M = 1.
- k_colsum_adamw<16, 64> (M > 128): section 4 at M = 129 over N = 1 .. 65 (1 .. 5 workgroups); the trainer at B = 26 (130 token rows).
- k_ln_wgrad_partial<1, 4>: dims 4, 36, 64, 128, 192, 256;  <2, 4>: 260, 384, 512;  <3, 4>: 768;  <4, 2>: 1024;  <8, 2>: 1028, 1280,
  2048 -- sections 6 and 7.  Dims 4, 36, 260 and 1028 leave lanes (4, 36: most of them) outside the row; the row sweep of section 6 runs
  1 .. 129 rows at one dim per look-ahead depth (R = 4: 36, 512; R = 2: 1024, 2048), so that a chunk ends on an odd row of R = 2 and on
  every residue of R = 4; k_ln_wgrad_finish adds 1, 2, 3, 4 and (section 7) 66 partials.

References: float64 for everything that rounds (the GEMM gradient under its per-element bound, dgamma under the fp32-relative rule of
test_gpu_grad_edges.within_fp32), the numpy float32 listings of test_vit_train_host (adamw_f32, chunked_colsum_f32) where the claim is
"bit for bit".  Nothing here can reach outside an allocation of its own: rows past M, columns past N and floats around every written
buffer are guard zones of the same tensor."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_grad_edges import LN_DIMS, within_fp32
from test_gpu_vit_train import _check_update, _state, make_trainer, oracle_gradients, plan_shape, rel_l2
from test_vit_train_host import adamw_f32, chunked_colsum_f32

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
LN_EPS = 1e-6
NAN = float("nan")
FRONT, BACK = 257, 256           # guard floats around a live range: the range starts an odd number of floats into its allocation
ND_ERR_ARG = -1
GS3 = 1.0 / 3.0


def gen(seed):
    return torch.Generator().manual_seed(seed)


def lib():
    from nested_diffusion_amd import _lib
    return _lib.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


def u32(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float32)
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(got, want, what):
    g, w = u32(got), u32(want)
    bad = np.nonzero(g.reshape(-1) != w.reshape(-1))[0]
    assert g.shape == w.shape and bad.size == 0, (what, int(bad.size), bad[:8].tolist())


class Guarded:
    """`n` live floats `front` floats into a buffer of NaNs told apart by their payload, `BACK` more behind them.  src: a CPU tensor copied
    into the live range (its shape is kept), or a number of floats, which stay poisoned."""

    def __init__(self, src, front=FRONT):
        shape = tuple(src.shape) if isinstance(src, torch.Tensor) else (int(src),)
        n = int(np.prod(shape))
        self.buf = torch.empty(front + n + BACK, dtype=torch.float32, device=DEV)
        self.buf.view(torch.int32)[:] = 0x7FC00000 + torch.arange(self.buf.numel(), dtype=torch.int32, device=DEV) % 4096
        self.t = self.buf[front:front + n].view(shape)
        if isinstance(src, torch.Tensor):
            self.t.copy_(src)
        self.front, self.n = front, n
        self.poison = self.buf.view(torch.int32).clone()
        assert self.t.data_ptr() == self.buf.data_ptr() + 4 * front and self.t.is_contiguous()

    @property
    def ptr(self):
        return self.t.data_ptr()

    def check(self, what):
        now = self.buf.view(torch.int32)
        lo, hi = self.front, self.front + self.n
        assert torch.equal(now[:lo], self.poison[:lo]), f"{what}: written in front of the buffer"
        assert torch.equal(now[hi:], self.poison[hi:]), f"{what}: written behind the buffer"

    def untouched(self):
        return torch.equal(self.buf.view(torch.int32), self.poison)


def odd(t):
    """a GPU copy of the CPU tensor t that starts one float into its allocation: 4-byte aligned and no more"""
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view


def grad_only(dy, x, gscale):
    from nested_diffusion_amd import ops
    return ops.gemm_tn_adamw(dy.to(DEV), x.to(DEV), None, None, None, None, gscale=gscale, return_grad=True)


# ---- 1. the GEMM gradient over M: every step and stage edge, zero padding, rows past M ----------------------------------------------------
M_SWEEP = [1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 95, 96, 97]
SWEEP_N, SWEEP_K = 33, 48


@functools.lru_cache(maxsize=None)
def sweep_inputs(M):
    g = gen(7000 + M)
    return torch.randn(M, SWEEP_N, generator=g), torch.randn(M, SWEEP_K, generator=g)


@functools.lru_cache(maxsize=None)
def sweep_grad(M):
    """the gradient-only launch on exactly sized tensors, computed once per M: what sections 1a, 1b and 1c compare with"""
    return grad_only(*sweep_inputs(M), GS3).cpu()


@pytest.mark.parametrize("M", M_SWEEP)
def test_gemm_gradient_m_sweep_and_zero_padding(M):
    """(a) (M + 2) 2^-24 sum_m |dy x| |gscale| per element against float64: one rounding per product, M - 1 sums, one scale.
    (b) dy and x padded with zero rows to 32 ceil(M / 32) + 32 rows give the same bits: adding 0 * 0 to an accumulator is exact, so the
    short last stage (ceil(left / 4) steps) and a full stage followed by a stage of zeros must agree."""
    dy, x = sweep_inputs(M)
    got = sweep_grad(M)
    assert tuple(got.shape) == (SWEEP_N, SWEEP_K)
    gs = float(np.float32(GS3))
    ref = dy.double().t() @ x.double() * gs
    bound = (M + 2) * U * (dy.double().abs().t() @ x.double().abs()) * gs
    err = (got.double() - ref).abs()
    print(f"M={M}: max |g - g64| = {float(err.max()):.3e}, max bound = {float(bound.max()):.3e}, worst err / bound = {float((err / bound).max()):.3f}")
    assert float((err - bound).max()) <= 0.0, (M, float((err - bound).max()))
    rows = 32 * ((M + 31) // 32) + 32
    dyp, xp = torch.zeros(rows, SWEEP_N), torch.zeros(rows, SWEEP_K)
    dyp[:M], xp[:M] = dy, x
    padded = grad_only(dyp, xp, GS3).cpu()
    assert torch.equal(padded, got), (M, rows, int((padded != got).sum()))


@pytest.mark.parametrize("M", [1, 3, 30, 33, 64])
def test_gemm_never_reads_rows_past_m(M):
    """dy and x are the first M rows of allocations whose 40 further rows are NaN: the last step of four rows (M = 1, 3, 30, 33) and the
    prefetch of the stage that follows a full one (M = 64: m1 == M) zero-fill in registers.  The bits of the exactly sized launch."""
    from nested_diffusion_amd import ops
    dy, x = sweep_inputs(M)
    views = []
    for t in (dy, x):
        buf = torch.full((M + 40, t.shape[1]), NAN, device=DEV)
        buf[:M] = t.to(DEV)
        view = buf[:M]
        assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() and bool(buf[M:].isnan().all())
        views.append(view)
    got = ops.gemm_tn_adamw(views[0], views[1], None, None, None, None, gscale=GS3, return_grad=True).cpu()
    assert bool(got.isfinite().all()), M
    assert torch.equal(got, sweep_grad(M)), M


# ---- 2. the GEMM's bits do not depend on the tile or the grid ----------------------------------------------------------------------------------
def _forward_and_backward_sums_differ(dy, x):
    """float32 sums over m of the float32 products dy[m, n] x[m, k], in the order m = 0 .. M - 1 and in the reverse: do they differ in
    at least one element?  (If the order could not be seen in these inputs, equal bits would say nothing about the order.)"""
    dy, x = dy.numpy(), x.numpy()
    fwd, bwd = np.zeros((dy.shape[1], x.shape[1]), np.float32), np.zeros((dy.shape[1], x.shape[1]), np.float32)
    for m in range(dy.shape[0]):
        fwd = fwd + dy[m][:, None] * x[m][None, :]
    for m in reversed(range(dy.shape[0])):
        bwd = bwd + dy[m][:, None] * x[m][None, :]
    return bool((fwd != bwd).any())


def test_gemm_bits_do_not_depend_on_the_tile_or_the_grid():
    """(M, N, K) = (70, 130, 144): a 3 x 3 grid whose last tiles hold 2 rows of G and 16 columns.  A block of G recomputed from the
    matching column slices of dy and x -- where it falls into other tiles, other waves' quadrants and another grid -- has the same bits:
    every element is one chain over m = 0 .. M - 1 whatever tile it falls in."""
    from nested_diffusion_amd import ops
    M, N, K = 70, 130, 144
    p = ops.gemm_tn_plan(N, K)
    assert (p["grid_n"], p["grid_k"]) == (3, 3) and N - 2 * p["tile_n"] == 2 and K - 2 * p["tile_k"] == 16
    g = gen(2)
    dy, x = torch.randn(M, N, generator=g), torch.randn(M, K, generator=g)
    blocks = [((64, 130), (64, 144)), ((129, 130), (128, 144)), ((5, 6), (0, 16))]
    for (n0, n1), (k0, k1) in blocks:
        assert _forward_and_backward_sums_differ(dy[:, n0:n1], x[:, k0:k1]), (n0, n1, k0, k1)
    G = grad_only(dy, x, GS3)
    for (n0, n1), (k0, k1) in blocks:
        part = grad_only(dy[:, n0:n1].contiguous(), x[:, k0:k1].contiguous(), GS3)
        assert tuple(part.shape) == (n1 - n0, k1 - k0)
        assert torch.equal(part, G[n0:n1, k0:k1]), ((n0, n1), (k0, k1), int((part != G[n0:n1, k0:k1]).sum()))


# ---- 3. the fused GEMM update on more than one tile, inside guard zones ------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["ragged", (64, 65, 64), (4, 64, 16)], ids=str)
def test_fused_gemm_update_inside_guard_zones(shape):
    """w, m, v and g_out each inside a poisoned buffer, 257 floats in (4-byte aligned, as the header promises and no more), dy and x one
    float in.  (t, lr) = (7, 1e-4) on a populated state: g_out is the gradient-only call's, w / m / v the float32 listing bit for bit,
    every guard float keeps its bits; then the same without g_out."""
    from nested_diffusion_amd import ops
    M, N, K = plan_shape(shape) if isinstance(shape, str) else shape
    g = gen(300 + M + N)
    dy, x = torch.randn(M, N, generator=g), torch.randn(M, K, generator=g)
    w0, m0, v0 = _state((N, K), True, g)
    a = ops.adamw_step(1e-4, 7)
    gscale = 1.0 / M
    only = grad_only(dy, x, gscale).cpu()
    we, me, ve = adamw_f32(w0.numpy(), m0.numpy(), v0.numpy(), only.numpy(), a)
    assert not np.array_equal(we, w0.numpy())
    dyd, xd = odd(dy), odd(x)
    for with_g in (True, False):
        w, m, v, go = Guarded(w0), Guarded(m0), Guarded(v0), Guarded(N * K)
        rc = lib().nd_gemm_tn_adamw(dyd.data_ptr(), xd.data_ptr(), w.ptr, m.ptr, v.ptr, go.ptr if with_g else None, M, N, K, gscale,
                                    ctypes.byref(a), stream())
        assert rc == 0, lib().nd_last_error()
        torch.cuda.synchronize()
        what = f"{(M, N, K)} g_out={with_g}"
        if with_g:
            same_bits(go.t.view(N, K), only, "g_out " + what)
        else:
            assert go.untouched(), what
        same_bits(m.t, me, "m " + what)
        same_bits(v.t, ve, "v " + what)
        same_bits(w.t, we, "w " + what)
        for name, gd in (("w", w), ("m", m), ("v", v), ("g_out", go)):
            gd.check(f"{name} {what}")


# ---- 4. the column sum over widths ------------------------------------------------------------------------------------------------------------
COLSUM_CASES = [(M, N) for M in (2, 129) for N in (1, 15, 16, 17, 63, 64, 65)] + [(2, 151296)]


@pytest.mark.parametrize("M,N", COLSUM_CASES)
def test_colsum_widths_bit_for_bit_inside_guard_zones(M, N):
    """One column, both sides of the 16-column workgroup of the narrow form (M = 129) and of the 64-column one (M = 2), and pos_embed's
    width at ViT-B/16, 197 * 768 = 151296 columns (2364 workgroups).  g_out is the documented order times float32(gscale), b / m / v the
    float32 listing, bit for bit; b, m, v and g_out sit 257 floats into poisoned buffers, dy one float into its own."""
    from nested_diffusion_amd import ops
    assert (M > 2 * ops.COLSUM_CHUNK) == (M == 129)
    g = gen(40 * N + M)
    dy = torch.randn(M, N, generator=g)
    b0, m0, v0 = _state((N,), True, g)
    G = chunked_colsum_f32(dy.numpy(), ops.COLSUM_CHUNK) * np.float32(GS3)
    if M == 129 and N >= 15:                                 # the chunked order is not the plain row order
        plain = np.zeros(N, np.float32)
        for r in range(M):
            plain = plain + dy[r].numpy()
        assert not np.array_equal(plain * np.float32(GS3), G)
    a = ops.adamw_step(1e-4, 7)
    be, me, ve = adamw_f32(b0.numpy(), m0.numpy(), v0.numpy(), G, a)
    b, m, v, go = Guarded(b0), Guarded(m0), Guarded(v0), Guarded(N)
    dyd = odd(dy)
    rc = lib().nd_colsum_adamw(dyd.data_ptr(), b.ptr, m.ptr, v.ptr, go.ptr, M, N, GS3, ctypes.byref(a), stream())
    assert rc == 0, lib().nd_last_error()
    torch.cuda.synchronize()
    for name, gd, want in (("g_out", go, G), ("m", m, me), ("v", v, ve), ("b", b, be)):
        same_bits(gd.t, want, f"{name} {(M, N)}")
        gd.check(f"{name} {(M, N)}")
    # the gradient-only launch: the same gradient, nothing else written
    go2 = Guarded(N)
    assert lib().nd_colsum_adamw(dyd.data_ptr(), None, None, None, go2.ptr, M, N, GS3, None, stream()) == 0
    torch.cuda.synchronize()
    same_bits(go2.t, G, f"gradient-only {(M, N)}")
    go2.check(f"gradient-only {(M, N)}")


# ---- 5. the AdamW listing at the edges of fp32, through each launch path ----------------------------------------------------------------------
G_EDGE = [0.0, 1e-30, -1e-30, 1e-20, -1e-20, 1.0, -1.0, 1e18, -1e18, 1e20, -1e20]
STATES = ("zero", "populated", "denormal v")
ADAMW_STEPS = {
    "t=1": dict(lr=1e-4, t=1, weight_decay=0.1),
    "t=1, wd=0": dict(lr=1e-4, t=1, weight_decay=0.0),
    "t=1e6": dict(lr=1e-3, t=10 ** 6, weight_decay=0.1),
    "lr=0": dict(lr=0.0, t=7, weight_decay=0.1),
    "betas": dict(lr=1e-4, t=3, weight_decay=0.1, betas=(0.5, 0.9)),
}


@pytest.mark.parametrize("step", list(ADAMW_STEPS))
def test_adamw_listing_at_the_edges_of_fp32_through_the_colsum(step):
    """nd_colsum_adamw at M = 1, gscale = 1: the gradient is the row of dy, bit for bit.  Every gradient of G_EDGE (zero; a square that
    underflows to 0; a denormal square; order one; 1e18, whose square is finite; 1e20, whose square is inf, where sqrt(v) = inf,
    m / denom = 0 and the weight is its decayed self, finite) on m = v = 0, on a populated state and on a denormal v.  w, m, v as uint32
    (so that a flushed denormal or the sign of a zero is seen) equal the numpy float32 listing, which keeps denormals (asserted)."""
    from nested_diffusion_amd import ops
    f32 = np.float32
    ng = len(G_EDGE)
    N = ng * len(STATES)
    gv = np.tile(np.array(G_EDGE, dtype=f32), len(STATES))
    si = np.repeat(np.arange(len(STATES)), ng)
    rng = np.random.RandomState(11)
    w0 = (0.1 * rng.randn(N)).astype(f32)
    m0 = np.where(si == 0, f32(0), (0.05 * rng.randn(N)).astype(f32)).astype(f32)
    v0 = np.select([si == 0, si == 1], [f32(0), (0.01 * rng.rand(N)).astype(f32) + f32(1e-6)], f32(1e-40)).astype(f32)
    assert 0 < v0[-1] < f32(2.0 ** -126)
    a = ops.adamw_step(**ADAMW_STEPS[step])
    if step == "t=1, wd=0" or step == "lr=0":
        assert a.decay == 1.0
    with np.errstate(all="ignore"):
        we, me, ve = adamw_f32(w0, m0, v0, gv, a)
        # the listing meets what it is meant to meet, and the host keeps denormals
        i20, i30, ibig = G_EDGE.index(1e-20), G_EDGE.index(1e-30), G_EDGE.index(1e20)
        assert gv[i30] * gv[i30] == 0 and 0 < gv[i20] * gv[i20] < f32(2.0 ** -126)
        assert 0 < ve[i20] < f32(2.0 ** -126), ve[i20]
        assert np.isinf(ve[ibig]) and np.isinf(ve[ibig + 1]) and np.isinf(ve[ng + ibig]) and np.isinf(ve[2 * ng + ibig])
    assert np.isfinite(we).all() and np.isfinite(me).all()
    for s in range(len(STATES)):                               # g g = inf: the weight is the decayed weight
        for j in (ibig, ibig + 1):
            assert we[s * ng + j] == w0[s * ng + j] * f32(a.decay)
    b, m, v, go = Guarded(torch.from_numpy(w0)), Guarded(torch.from_numpy(m0)), Guarded(torch.from_numpy(v0)), Guarded(N)
    dyd = odd(torch.from_numpy(gv).view(1, N))
    rc = lib().nd_colsum_adamw(dyd.data_ptr(), b.ptr, m.ptr, v.ptr, go.ptr, 1, N, 1.0, ctypes.byref(a), stream())
    assert rc == 0, lib().nd_last_error()
    torch.cuda.synchronize()
    bad = []
    for name, gd, want in (("g", go, gv), ("m", m, me), ("v", v, ve), ("w", b, we)):
        got = gd.t.cpu().numpy()
        for i in np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]:
            bad.append((name, STATES[si[i]], float(gv[i]), float(w0[i]), float(m0[i]), float(v0[i]), float(got[i]), float(want[i])))
        gd.check(f"{name} {step}")
    assert not bad, (len(bad), bad[:12])
    if step == "lr=0":
        same_bits(b.t, w0, "lr = 0 leaves the weight's bits")


@pytest.mark.parametrize("step", ["t=1, wd=0", "t=1e6"])
def test_adamw_listing_without_decay_and_at_large_t_through_the_gemm_and_the_layernorm(step):
    """the two steps no other test sends through nd_gemm_tn_adamw (15, 17, 48) and nd_layernorm_wgrad_adamw (15, 128): the update is the
    float32 listing of each call's own returned gradient, bit for bit"""
    from nested_diffusion_amd import ops
    a = ops.adamw_step(**ADAMW_STEPS[step])
    assert (a.decay == 1.0) == (step == "t=1, wd=0")
    lr = ADAMW_STEPS[step]["lr"]
    g = gen(55)
    M, N, K = 15, 17, 48
    dy, x = torch.randn(M, N, generator=g), torch.randn(M, K, generator=g)
    w0, m0, v0 = _state((N, K), True, g)
    w, m, v = w0.to(DEV), m0.to(DEV), v0.to(DEV)
    G = ops.gemm_tn_adamw(dy.to(DEV), x.to(DEV), w, m, v, a, gscale=1.0 / M, return_grad=True)
    assert torch.equal(G, grad_only(dy, x, 1.0 / M))
    _check_update(w, m, v, w0, m0, v0, G.cpu().numpy(), a, lr)
    rows, dim = 15, 128
    xl, gl = torch.randn(rows, dim, generator=g) * 1.5 + 0.3, torch.randn(rows, dim, generator=g)
    (gam0, mg0, vg0), (bet0, mb0, vb0) = _state((dim,), True, g), _state((dim,), True, g)
    gam, bet, mg, vg, mb, vb = (t.clone().to(DEV) for t in (gam0, bet0, mg0, vg0, mb0, vb0))
    dg, db = ops.layernorm_wgrad_adamw(xl.to(DEV), gl.to(DEV), LN_EPS, gam, bet, mg, vg, mb, vb, a, gscale=GS3, return_grad=True)
    _check_update(gam, mg, vg, gam0, mg0, vg0, dg.cpu().numpy(), a, lr)
    _check_update(bet, mb, vb, bet0, mb0, vb0, db.cpu().numpy(), a, lr)


# ---- 6. the LayerNorm parameter gradient: every instantiation, every chunk edge -----------------------------------------------------------------
LN_ROW_SWEEP = [1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129]
LN_CASES = [(rows, dim) for dim in LN_DIMS for rows in (1, 3, 17, 197)]
LN_CASES += [(rows, dim) for dim in (36, 512, 1024, 2048) for rows in LN_ROW_SWEEP if (rows, dim) not in LN_CASES]


def ln_autograd(x, g, dtype):
    """(dgamma, dbeta) of sum(layer_norm(x) * g) by torch autograd in `dtype`, as float64"""
    dim = x.shape[1]
    ga, be = torch.ones(dim, dtype=dtype, requires_grad=True), torch.zeros(dim, dtype=dtype, requires_grad=True)
    (F.layer_norm(x.to(dtype), (dim,), ga, be, LN_EPS) * g.to(dtype)).sum().backward()
    return ga.grad.double(), be.grad.double()


def ln_grads(x, g, gscale):
    from nested_diffusion_amd import ops
    dg, db = ops.layernorm_wgrad_adamw(x.to(DEV), g.to(DEV), LN_EPS, None, None, None, None, None, None, None, gscale=gscale, return_grad=True)
    return dg.cpu(), db.cpu()


def gpu_xhat(x):
    """the forward kernel's xhat: nd_layernorm with gamma = 1, beta = 0 (a product with 1 and a sum with 0 are exact, fused or not)"""
    from nested_diffusion_amd import ops
    dim = x.shape[1]
    return ops.layernorm(x.to(DEV), torch.ones(dim, device=DEV), torch.zeros(dim, device=DEV), LN_EPS).cpu().numpy()


def plain_colsum_f32(terms):
    acc = np.zeros(terms.shape[1], np.float32)
    for r in range(terms.shape[0]):
        acc = acc + terms[r]
    return acc


@pytest.mark.parametrize("rows,dim", LN_CASES)
def test_layernorm_parameter_gradient_every_instantiation_and_chunk_edge(rows, dim):
    """dbeta: the documented order of g times float32(gscale), bit for bit.  dgamma: the fp32-relative rule against float64 autograd,
    and the documented order of the float32 products g * xhat, xhat taken from nd_layernorm (gamma = 1, beta = 0) -- the header's "xhat
    recomputed as nd_layernorm does" taken at its word -- bit for bit (measured on an MI355X: it holds at all 92 cases, so it is what
    this test asserts and no per-element bound stands in for it).  From 129 rows on the chunked order of these very terms is not the
    plain row order (asserted), so the order is seen.  Then one fused call on a populated state: the same gradients, the listing's update."""
    from nested_diffusion_amd import ops
    chunk = ops.COLSUM_CHUNK
    gn = gen(rows * 10000 + dim)
    x = torch.randn(rows, dim, generator=gn) * 1.5 + 0.3
    g = torch.randn(rows, dim, generator=gn)
    gs = np.float32(GS3)
    dg, db = ln_grads(x, g, GS3)
    same_bits(db, chunked_colsum_f32(g.numpy(), chunk) * gs, f"dbeta {(rows, dim)}")
    dg64, _ = ln_autograd(x, g, torch.float64)
    dg32, _ = ln_autograd(x, g, torch.float32)
    err, err32 = rel_l2(dg, dg64 * float(gs)), rel_l2(dg32, dg64)
    terms = g.numpy() * gpu_xhat(x)
    assert terms.dtype == np.float32
    want = chunked_colsum_f32(terms, chunk) * gs
    print(f"({rows}, {dim}): dgamma rel L2 {err:.3e} (torch fp32 {err32:.3e}); elements off the documented order: "
          f"{int((u32(dg) != u32(want)).sum())}")
    assert bool(dg.isfinite().all()) and within_fp32(err, err32, 1e-5), (rows, dim, err, err32)
    same_bits(dg, want, f"dgamma in the documented order {(rows, dim)}")
    if rows >= 129:
        for what, t in (("g", g.numpy()), ("g xhat", terms)):
            assert not np.array_equal(plain_colsum_f32(t), chunked_colsum_f32(t, chunk)), (what, rows, dim)
    sg = gen(dim)
    (gam0, mg0, vg0), (bet0, mb0, vb0) = _state((dim,), True, sg), _state((dim,), True, sg)
    gam, bet, mg, vg, mb, vb = (t.clone().to(DEV) for t in (gam0, bet0, mg0, vg0, mb0, vb0))
    a = ops.adamw_step(1e-4, 7)
    dg2, db2 = ops.layernorm_wgrad_adamw(x.to(DEV), g.to(DEV), LN_EPS, gam, bet, mg, vg, mb, vb, a, gscale=GS3, return_grad=True)
    assert torch.equal(dg2.cpu(), dg) and torch.equal(db2.cpu(), db)
    _check_update(gam, mg, vg, gam0, mg0, vg0, dg.numpy(), a, 1e-4)
    _check_update(bet, mb, vb, bet0, mb0, vb0, db.numpy(), a, 1e-4)


def edge_rows(dim, all_constant):
    gn = gen(900 + dim)
    x = torch.randn(70, dim, generator=gn) * 1.5 + 0.3
    g = torch.randn(70, dim, generator=gn)
    if all_constant:
        x = (0.7 + 0.013 * torch.arange(70, dtype=torch.float32))[:, None].expand(70, dim).contiguous()
    else:
        x[0], x[65] = 0.7, -3.3
        x[1] = 1e3 + 1e-2 * torch.randn(dim, generator=gn)
        g[2] = 0
    return x, g


@pytest.mark.parametrize("dim", [36, 768, 2048])
def test_layernorm_parameter_gradient_edge_rows(dim):
    """70 rows (two chunks): row 0 and row 65 constant (rstd = eps^-1/2 = 1000), row 1 of mean 1e3 and spread 1e-2, row 2 with g = 0.
    dgamma finite and under the fp32-relative rule, dbeta the documented order bit for bit."""
    from nested_diffusion_amd import ops
    x, g = edge_rows(dim, False)
    dg, db = ln_grads(x, g, GS3)
    gs = np.float32(GS3)
    same_bits(db, chunked_colsum_f32(g.numpy(), ops.COLSUM_CHUNK) * gs, f"dbeta {dim}")
    dg64, _ = ln_autograd(x, g, torch.float64)
    dg32, _ = ln_autograd(x, g, torch.float32)
    err, err32 = rel_l2(dg, dg64 * float(gs)), rel_l2(dg32, dg64)
    print(f"dim={dim} edge rows: dgamma rel L2 {err:.3e}, torch fp32 {err32:.3e}")
    assert bool(dg.isfinite().all()) and within_fp32(err, err32, 1e-5), (dim, err, err32)


@pytest.mark.parametrize("dim", [36, 768, 2048])
def test_layernorm_parameter_gradient_of_constant_rows(dim):
    """Every row constant: xhat, and with it dgamma, is 0 in exact arithmetic, so the rule gets an absolute floor: ||dgamma|| against
    the larger of 4 ||torch float32 dgamma|| and ||2^-24 sum_r |g| 1000 2^-23|| (one ulp of xhat at rstd = eps^-1/2), all times gscale.
    Which of the two is the bound: the first, by six orders of magnitude (4 x torch float32 is 2.0e-3, 9.4e-3 and 1.5e-2 at dims 36,
    768 and 2048, the floor 7.8e-10, 3.7e-9 and 6.0e-9).  Measured on an MI355X the kernel needs neither: ||dgamma|| is exactly 0 at all
    three dims, because nd_ln_stats' correction c = sum(x - mean) / dim makes (x - mean) - c exactly 0 on a constant row.  dbeta stays
    the documented order bit for bit."""
    from nested_diffusion_amd import ops
    x, g = edge_rows(dim, True)
    dg, db = ln_grads(x, g, GS3)
    gs = np.float32(GS3)
    same_bits(db, chunked_colsum_f32(g.numpy(), ops.COLSUM_CHUNK) * gs, f"dbeta {dim}")
    dg32, _ = ln_autograd(x, g, torch.float32)
    got = float(dg.double().norm())
    yard = 4 * float(dg32.norm()) * float(gs)
    floor = float((U * g.double().abs().sum(0) * 1000 * 2.0 ** -23).norm()) * float(gs)
    print(f"dim={dim} constant rows: ||dgamma|| = {got:.3e}, 4 x torch fp32 = {yard:.3e}, floor = {floor:.3e}")
    assert bool(dg.isfinite().all()) and got <= max(yard, floor), (dim, got, yard, floor)


# ---- 7. the LayerNorm workspace -----------------------------------------------------------------------------------------------------------------
def ln_raw(x, g, ws_ptr, ws_bytes, dg_ptr, db_ptr, gscale=GS3):
    rows, dim = x.shape
    return lib().nd_layernorm_wgrad_adamw(x.data_ptr(), g.data_ptr(), None, None, None, None, None, None, dg_ptr, db_ptr, rows, dim, LN_EPS,
                                          gscale, None, ws_ptr, ws_bytes, stream())


@pytest.mark.parametrize("rows,dim", [(1, 4), (65, 260), (129, 2048)])
def test_layernorm_workspace_is_exactly_the_bytes_the_library_names(rows, dim):
    """The workspace is nd_layernorm_wgrad_workspace_bytes long and no longer, 16-byte aligned inside a poisoned buffer and NaN itself:
    the results are finite and the ops call's (k_ln_wgrad_finish reads only partials that were written), the guards on both sides and
    those of dgamma / dbeta keep their bits.  Four bytes fewer are refused before any launch."""
    need = lib().nd_layernorm_wgrad_workspace_bytes(rows, dim)
    assert need == ((rows + 63) // 64) * 2 * dim * 4
    gn = gen(rows + dim)
    x, g = torch.randn(rows, dim, generator=gn) * 1.5 + 0.3, torch.randn(rows, dim, generator=gn)
    want_dg, want_db = ln_grads(x, g, GS3)
    xd, gd = x.to(DEV), g.to(DEV)
    ws, dg, db = Guarded(need // 4, front=256), Guarded(dim), Guarded(dim)
    assert ws.ptr % 16 == 0 and bool(ws.t.isnan().all())
    rc = ln_raw(xd, gd, ws.ptr, need - 4, dg.ptr, db.ptr)
    torch.cuda.synchronize()
    msg = lib().nd_last_error().decode()
    assert rc == ND_ERR_ARG and "workspace" in msg and f"{need} needed" in msg, (rc, msg)
    assert ws.untouched() and dg.untouched() and db.untouched()
    rc = ln_raw(xd, gd, ws.ptr, need, dg.ptr, db.ptr)
    assert rc == 0, lib().nd_last_error()
    torch.cuda.synchronize()
    assert bool(dg.t.isfinite().all()) and bool(db.t.isfinite().all()) and bool(ws.t.isfinite().all())
    same_bits(dg.t, want_dg, f"dgamma {(rows, dim)}")
    same_bits(db.t, want_db, f"dbeta {(rows, dim)}")
    for name, gd_ in (("workspace", ws), ("dgamma", dg), ("dbeta", db)):
        gd_.check(f"{name} {(rows, dim)}")


def test_layernorm_workspace_grows_past_a_mebibyte():
    """(4161, 2048): 66 chunks, 1081344 bytes of partials, more than the 1 MiB ops._workspace starts from.  Through ops on a fresh
    stream (whose cache entry does not exist yet, so that it is created at the larger size) and through the ABI on an exactly sized
    workspace: the same bits, dbeta the documented order."""
    from nested_diffusion_amd import ops
    rows, dim = 4161, 2048
    need = lib().nd_layernorm_wgrad_workspace_bytes(rows, dim)
    assert need == 66 * 2 * dim * 4 and need > 1 << 20
    gn = gen(4161)
    x, g = torch.randn(rows, dim, generator=gn) * 1.5 + 0.3, torch.randn(rows, dim, generator=gn)
    xd, gd = x.to(DEV), g.to(DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    key = (str(xd.device), side.cuda_stream)
    assert key not in ops._ws_cache
    with torch.cuda.stream(side):
        dg, db = ops.layernorm_wgrad_adamw(xd, gd, LN_EPS, None, None, None, None, None, None, None, gscale=GS3, return_grad=True)
    side.synchronize()
    assert ops._ws_cache[key].numel() >= need
    ws, rdg, rdb = Guarded(need // 4, front=256), Guarded(dim), Guarded(dim)
    assert ln_raw(xd, gd, ws.ptr, need, rdg.ptr, rdb.ptr) == 0, lib().nd_last_error()
    torch.cuda.synchronize()
    same_bits(rdg.t, dg, "dgamma")
    same_bits(rdb.t, db, "dbeta")
    for name, gd_ in (("workspace", ws), ("dgamma", rdg), ("dbeta", rdb)):
        gd_.check(name)
    same_bits(db, chunked_colsum_f32(g.numpy(), ops.COLSUM_CHUNK) * np.float32(GS3), "dbeta against the documented order")
    del ops._ws_cache[key]


# ---- 8. the trainer at batches that cross a chunk ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [13, 26])
def test_trainer_step_at_chunk_crossing_batches(B):
    """make_trainer(128, 2, 32): 5 tokens an image.  B = 13: 65 token rows, one past a chunk of the column sums and one past two LDS
    stages of the GEMM; B = 26: 130 rows, the narrow column-sum form.  One step from a fresh trainer is the float32 listing of
    gradients() for every parameter, m and v, bit for bit; gradients() follows float64 autograd through the oracle."""
    from nested_diffusion_amd import ops
    trainer, vp = make_trainer(128, 2, 32)
    g = gen(80 + B)
    x, labels = torch.rand(B, 3, 32, 32, generator=g), torch.randint(0, 2, (B,), generator=g)
    assert B * 5 in (ops.COLSUM_CHUNK + 1, 2 * ops.COLSUM_CHUNK + 2)
    w0 = trainer.state_dict()
    m0 = {k: t.cpu().clone() for k, t in trainer.m.items()}
    v0 = {k: t.cpu().clone() for k, t in trainer.v.items()}
    grads, loss, logits = trainer.gradients(x, labels)
    ref, _ = oracle_gradients(vp, x, labels, 2, 2)
    worst = {k: rel_l2(grads[k].cpu(), ref[k]) for k in vp}
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:3]
    print(f"B {B}: largest rel L2 {top}")
    assert sorted(grads) == sorted(vp) and top[0][1] <= 1e-4, top
    loss_sum, n_correct = trainer.step(x, labels)
    assert trainer.t == 1 and float(loss_sum) == float(loss.sum()) and int(n_correct) == int((logits.argmax(1).cpu() == labels).sum())
    a = ops.adamw_step(1e-4, 1, 0.1)
    w1 = trainer.state_dict()
    for k in vp:
        we, me, ve = adamw_f32(w0[k].numpy(), m0[k].numpy(), v0[k].numpy(), grads[k].cpu().numpy(), a)
        np.testing.assert_array_equal(trainer.m[k].cpu().numpy(), me, err_msg=k)
        np.testing.assert_array_equal(trainer.v[k].cpu().numpy(), ve, err_msg=k)
        np.testing.assert_array_equal(w1[k].numpy(), we, err_msg=k)
        assert not np.array_equal(we, w0[k].numpy()), k
