"""The listings of include/nested_diffusion.h, "the input gradient of the ensemble", restated in numpy float32 (no GPU, no library): one
rounded fp32 operation per line, in the header's order, so that a kernel of csrc/nd_ensemble_grad.hip can be compared BIT FOR BIT.
tests/test_ensemble_grad_listing_host.py shows each restatement to agree with float64 within its counted bound;
tests/test_gpu_ensemble_grad_edges.py compares the kernels with them.

Every array operand is made float32 on entry and every scalar an np.float32, so that numpy never widens an intermediate: `a * b`, `a / b`
and np.sqrt(a) on float32 are IEEE operations, correctly rounded.  The fused multiply-add of the coefficient form is the C library's fmaf
(libm.so.6 through ctypes); HAVE_FMAF is False where it cannot be loaded, and reverse_step_coef_f32 then raises."""
import ctypes

import numpy as np

F = np.float32
U = 2.0 ** -24                       # unit roundoff of fp32
RSTEP_INIT, RSTEP_UPDATE, RSTEP_LAST = 0, 1, 2
ONE = F(1.0)


def _load_fmaf():
    try:
        f = ctypes.CDLL("libm.so.6").fmaf
    except (OSError, AttributeError):
        return None
    f.argtypes = [ctypes.c_float, ctypes.c_float, ctypes.c_float]
    f.restype = ctypes.c_float
    return f


_FMAF = _load_fmaf()
HAVE_FMAF = _FMAF is not None
FMAF_MISSING = "libm.so.6 with fmaf could not be loaded through ctypes"


def fmaf(a, b, c):
    """round(a * b + c), ONE rounding, elementwise over float32 operands (scalars broadcast)."""
    if _FMAF is None:
        raise RuntimeError(FMAF_MISSING)
    a, b, c = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F), np.asarray(c, F))
    out = np.empty(a.shape, F)
    of, fn = out.reshape(-1), _FMAF
    for i, (x, y, z) in enumerate(zip(a.reshape(-1).tolist(), b.reshape(-1).tolist(), c.reshape(-1).tolist())):
        of[i] = fn(x, y, z)
    return out


def _f(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F))


def _layout(new, ymean, ldo):
    """[M, ldo]: columns 0 .. C-1 the new state, C .. 2C-1 ymean[r % B] (ldo >= 2C), the rest +0."""
    M, C = new.shape
    B = ymean.shape[0]
    assert ldo == C or ldo >= 2 * C
    out = np.zeros((M, ldo), F)
    out[:, :C] = new
    if ldo >= 2 * C:
        out[:, C:2 * C] = ymean[np.arange(M) % B]
    return out


def posterior_f32(y, ym, eps, z, alpha_t, s_t, s_tm1):
    """nd_posterior of csrc/nd_step.hpp, line by line; y, ym, eps, z: float32 arrays of one shape."""
    alpha_t, s_t, s_tm1 = F(alpha_t), F(s_t), F(s_tm1)
    st2 = s_t * s_t
    t0 = ONE - st2
    sab_t = np.sqrt(t0)
    stm2 = s_tm1 * s_tm1
    t1 = ONE - stm2
    sab_tm1 = np.sqrt(t1)
    sa = np.sqrt(alpha_t)
    oma = ONE - alpha_t
    g0 = oma * sab_tm1
    g0 = g0 / st2
    g1 = stm2 * sa
    g1 = g1 / st2
    t2 = sab_t - ONE
    t3 = sa + sab_tm1
    g2 = t2 * t3
    g2 = g2 / st2
    g2 = ONE + g2
    y0r = y0_reparam_given_sab_f32(y, ym, eps, s_t, sab_t)
    m = g0 * y0r
    t4 = g1 * y
    m = m + t4
    t5 = g2 * ym
    m = m + t5
    bh = stm2 / st2
    bh = bh * oma
    sb = np.sqrt(bh)
    t6 = sb * z
    return m + t6


def y0_reparam_given_sab_f32(y, ym, eps, s_t, sab_t):
    """1.0f / sab_t * (y - (1.0f - sab_t) * ymean - eps * s_t): seven operations."""
    inv = ONE / sab_t
    w = ONE - sab_t
    a = w * ym
    a = y - a
    b = eps * s_t
    a = a - b
    return inv * a


def y0_reparam_f32(y, ym, eps, s_t):
    """nd_y0_reparam of csrc/nd_step.hpp."""
    s_t = F(s_t)
    st2 = s_t * s_t
    t0 = ONE - st2
    sab_t = np.sqrt(t0)
    return y0_reparam_given_sab_f32(y, ym, eps, s_t, sab_t)


def reverse_step_f32(mode, y, ymean, eps, z, alpha_t, s_t, s_tm1, ldo):
    """nd_reverse_step: y [M, ldy >= C] (its first C columns), ymean [B, C], eps, z [M, C] (the ones the mode does not read may be None);
    out [M, ldo] = [new state, ymean[r % B], 0 ..]."""
    ymean = _f(ymean)
    B, C = ymean.shape
    src = z if mode == RSTEP_INIT else y
    M = np.asarray(src).shape[0]
    ym = ymean[np.arange(M) % B]
    if mode == RSTEP_INIT:
        new = _f(z) + ym
    elif mode == RSTEP_UPDATE:
        new = posterior_f32(_f(y)[:, :C], ym, _f(eps), _f(z), alpha_t, s_t, s_tm1)
    elif mode == RSTEP_LAST:
        new = y0_reparam_f32(_f(y)[:, :C], ym, _f(eps), s_t)
    else:
        raise ValueError(f"unknown mode {mode}")
    return _layout(new, ymean, ldo)


def reverse_step_coef_f32(y, ymean, eps, z, cy, cm, ce, cz, ldo):
    """nd_reverse_step_coef: fmaf(cz, z, fmaf(ce, eps, fmaf(cm, ymean[r % B], cy * y))); z None: 0 is the draw."""
    ymean = _f(ymean)
    B, C = ymean.shape
    y = _f(y)[:, :C]
    M = y.shape[0]
    ym = ymean[np.arange(M) % B]
    zz = np.zeros((M, C), F) if z is None else _f(z)
    p = F(cy) * y
    v = fmaf(F(cm), ym, p)
    v = fmaf(F(ce), _f(eps), v)
    v = fmaf(F(cz), zz, v)
    return _layout(v, ymean, ldo)


def reverse_step_bwd_f32(g, C, cy, cm, ce, dymean_before, lda, want_deps):
    """nd_reverse_step_bwd: g [M, ldg], dymean_before [B, C].  Returns (deps [M, C] or None, dyadd [M, lda] or None (lda None),
    dymean [B, C]): acc = 0; per trial in trial order acc = acc + (cm * g), then acc = acc + g[C + c] (ldg >= 2C); dymean = before + acc."""
    g, before = _f(g), _f(dymean_before)
    cy, cm, ce = F(cy), F(cm), F(ce)
    M, ldg = g.shape
    B = before.shape[0]
    assert before.shape[1] == C and M % B == 0 and (ldg == C or ldg >= 2 * C)
    deps = ce * g[:, :C] if want_deps else None
    dyadd = None
    if lda is not None:
        dyadd = np.zeros((M, lda), F)
        dyadd[:, :C] = cy * g[:, :C]
    acc = np.zeros((B, C), F)
    for trial in range(M // B):
        rows = g[trial * B:(trial + 1) * B]
        t = cm * rows[:, :C]
        acc = acc + t
        if ldg >= 2 * C:
            acc = acc + rows[:, C:2 * C]
    return deps, dyadd, before + acc


def softmax_bwd_f32(p, dp):
    """nd_softmax_bwd on [rows, C]: dot = 0; dot = dot + (dp[c] * p[c]) in class order; dlogits[c] = p[c] * (dp[c] - dot)."""
    p, dp = _f(p), _f(dp)
    rows, C = p.shape
    dot = np.zeros(rows, F)
    for c in range(C):
        t = dp[:, c] * p[:, c]
        dot = dot + t
    d = dp - dot[:, None]
    return p * d


def cond_mul_f32(s, mul):
    """nd_cond_mul: y[r] = s[r] * mul[r % B]."""
    s, mul = _f(s), _f(mul)
    return s * mul[np.arange(s.shape[0]) % mul.shape[0]]


def cond_act_bwd_f32(dh, h, a_t, mul, prev, B):
    """nd_cond_act_bwd.  Returns (du, exact, dmul_acc).  sg = -expm1f(-h) is a library function, not a rounded operation, so du is
    restated only where sg is 1 by the listing: everywhere with h None, and where h > 20.  `exact` [M, N] marks those elements; du holds
    (g * 1) * a_t there and NaN elsewhere, and is None when no element is exact (the 10 U rule of tests/test_gpu_ensemble_grad.py is the
    check there).  dmul_acc [B, N] = prev + acc, acc = 0 then acc = acc + (dh * h) over the image's trials in trial order: always exact
    (None without mul)."""
    dh, a_t = _f(dh), _f(a_t)
    M, N = dh.shape
    assert M % B == 0
    exact = np.ones((M, N), bool) if h is None else _f(h) > F(20.0)
    g = dh if mul is None else dh * _f(mul)[np.arange(M) % B]
    du = None
    if exact.any():
        du = np.where(exact, g * a_t[None, :], F(np.nan)).astype(F)
    acc_out = None
    if mul is not None:
        h = _f(h)
        acc = np.zeros((B, N), F)
        for trial in range(M // B):
            t = dh[trial * B:(trial + 1) * B] * h[trial * B:(trial + 1) * B]
            acc = acc + t
        acc_out = _f(prev) + acc
    return du, exact, acc_out
