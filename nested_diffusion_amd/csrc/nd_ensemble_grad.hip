// nd_ensemble_grad.hip -- what the input gradient THROUGH THE SAMPLER has beyond nd_linear / nd_linear_bwd (include/nested_diffusion.h:
// "the input gradient of the ensemble"; the chain: nested_diffusion_amd/ensemble_grad.py).  gfx950 only, all arithmetic fp32.
//   k_cond_mul              y1 = s1 (.) xe[r % B]: the product of latent_model.py:177, kept apart from nd_linear's epilogue so that s1 stays
//   k_cond_act_bwd          the eval-mode backward of one ConditionalLinear + BatchNorm + softplus block, from the taped softplus OUTPUT
//   k_reverse_step          y_T = z + y_T_mean, p_sample, p_sample_t_1to0 on [M, C] (nd_step.hpp's nd_posterior / nd_y0_reparam, shared)
//   k_reverse_step_coef     one step of a sampler plan (strided / eta) on [M, C]: nd_step.hpp's nd_coef_update, shared with the sampler
//   k_reverse_step_bwd      the backward of one such step: it is affine, three host-formed coefficients
//   k_aggregate_xent_bwd    -log(mean_s softmax(-(y0_s - 1)^2 / tau))[label] and its gradient at every sample
//   k_softmax_bwd           dlogits = p (.) (dp - sum_c dp p)
//
// All of them are elementwise, row-streaming kernels over at most a few MB (M <= 128 rows of F <= 4096 floats; the [M, C] state is a few
// hundred floats): they are bound by launch latency, not by bandwidth, so the loads are plain coalesced dwords -- consecutive lanes read
// consecutive columns, no alignment demand on N -- and no LDS is used.  A thread of the two block kernels owns ONE column of ONE image and
// walks that image's trials in order: the scale a_t[n] and the xe[b, n] operand are loaded once and stay in registers, and the sum over
// the trials is a serial chain in trial order inside one thread: no atomics, the same bits on every run.  The aggregation kernels are
// instantiated per class count (1 .. 16) so that the per-class arrays are registers, not scratch.
#include "nd_host.hpp"
#include "nd_step.hpp"

#include <cmath>

namespace {

constexpr int EG_MAX_C = 16;     // nd_aggregate's ND_AGG_MAX_C

// sigma(z) of a softplus block from its OUTPUT h = softplus(z): 1 - exp(-h) = sigma(z) exactly (h = log(1 + e^z)), evaluated as
// -expm1(-h) -- the plain 1 - exp(-h) cancels to 0 once exp(-h) rounds to 1 (z <~ -16) -- and 1 above the threshold, where softplus is
// the identity (h > 20 exactly when z > 20: softplus(20) rounds to 20).
__device__ __forceinline__ float eg_sigma_from_softplus(float h) { return h > 20.0f ? 1.0f : -expm1f(-h); }

__global__ __launch_bounds__(256) void k_cond_mul(const float* __restrict__ s, const float* __restrict__ mul, float* __restrict__ y, int M, int N,
                                                  int B) {
    const int n = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (n >= N) return;
    const float x = mul[(size_t)b * N + n];
    for (int r = b; r < M; r += B) y[(size_t)r * N + n] = s[(size_t)r * N + n] * x;
}

__global__ __launch_bounds__(256) void k_cond_act_bwd(const float* dh, const float* __restrict__ h, const float* __restrict__ a_t,
                                                      const float* __restrict__ mul, float* du, float* __restrict__ dmul_acc, int M, int N, int B) {
#pragma clang fp contract(off)
    const int n = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (n >= N) return;
    const float a = a_t[n];
    const float x = mul ? mul[(size_t)b * N + n] : 1.0f;
    float acc = 0.f;
    for (int r = b; r < M; r += B) {                      // the image's trials in order: r = trial * B + b
        const size_t i = (size_t)r * N + n;
        const float d = dh[i];
        const float hv = h ? h[i] : 0.f;
        const float sg = h ? eg_sigma_from_softplus(hv) : 1.0f;
        const float g = mul ? d * x : d;
        du[i] = (g * sg) * a;
        if (mul) acc = acc + d * hv;
    }
    if (mul) dmul_acc[(size_t)b * N + n] = dmul_acc[(size_t)b * N + n] + acc;
}

// mode: ND_RSTEP_INIT / ND_RSTEP_UPDATE / ND_RSTEP_LAST.  One thread per output element (r, c) of the [M, ldo] output: c < C the new state,
// C <= c < 2C (ldo >= 2C: lin1's input [y_t, yhat, 0 ..]) y_T_mean[r % B], beyond that zeros.
__global__ __launch_bounds__(256) void k_reverse_step(int mode, const float* __restrict__ y, int ldy, const float* __restrict__ ymean,
                                                      const float* __restrict__ eps, const float* __restrict__ z, float* __restrict__ out, int ldo, int M,
                                                      int B, int C, float alpha_t, float s_t, float s_tm1) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= M * ldo) return;
    const int r = e / ldo, c = e - r * ldo, b = r % B;
    float v = 0.f;
    if (c < C) {
        const float ym = ymean[b * C + c];
        if (mode == ND_RSTEP_INIT) v = z[r * C + c] + ym;
        else if (mode == ND_RSTEP_UPDATE) v = nd_posterior(y[r * ldy + c], ym, eps[r * C + c], z[r * C + c], alpha_t, s_t, s_tm1);
        else v = nd_y0_reparam(y[r * ldy + c], ym, eps[r * C + c], s_t);
    } else if (c < 2 * C) {
        v = ymean[b * C + (c - C)];
    }
    out[e] = v;
}

// k_reverse_step's layouts with the update in coefficient form (a sampler plan's step: nd_step.hpp's nd_coef_update, the device function
// of the sampler's own coefficient kernels); z null: no draw is read (the step's cz is 0: the last step, or eta = 0).
__global__ __launch_bounds__(256) void k_reverse_step_coef(const float* __restrict__ y, int ldy, const float* __restrict__ ymean,
                                                           const float* __restrict__ eps, const float* __restrict__ z, float* __restrict__ out, int ldo,
                                                           int M, int B, int C, float cy, float cm, float ce, float cz) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= M * ldo) return;
    const int r = e / ldo, c = e - r * ldo, b = r % B;
    float v = 0.f;
    if (c < C) v = nd_coef_update(y[r * ldy + c], ymean[b * C + c], eps[r * C + c], z ? z[r * C + c] : 0.f, cy, cm, ce, cz);
    else if (c < 2 * C) v = ymean[b * C + (c - C)];
    out[e] = v;
}

// One thread per (image b, class c): the image's trials in order.  g [M, ldg]: columns 0 .. C-1 are dL/dy_{t-1}; with ldg >= 2C columns
// C .. 2C-1 are the yhat half of the previous trunk backward's lin1 gradient, which joins dymean here.
__global__ __launch_bounds__(256) void k_reverse_step_bwd(const float* __restrict__ g, int ldg, float cy, float cm, float ce, float* __restrict__ deps,
                                                          float* __restrict__ dyadd, int lda, float* __restrict__ dymean, int M, int B, int C) {
#pragma clang fp contract(off)
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= B * C) return;
    const int b = e / C, c = e - b * C;
    const bool hat = ldg >= 2 * C;
    float acc = 0.f;
    for (int r = b; r < M; r += B) {
        const float gv = g[r * ldg + c];
        if (deps) deps[r * C + c] = ce * gv;
        if (dyadd) {
            dyadd[r * lda + c] = cy * gv;
            for (int cc = C + c; cc < lda; cc += C) dyadd[r * lda + cc] = 0.f;
        }
        acc = acc + cm * gv;
        if (hat) acc = acc + g[r * ldg + C + c];
    }
    dymean[e] = dymean[e] + acc;
}

// One thread per image b.  The first pass is k_aggregate's (csrc/nd_report.hip) operation for operation, so P has nd_aggregate's bits; the
// second pass forms every sample's probabilities again (the same operations: the same values) instead of keeping S x C of them.
template <int C>
__global__ __launch_bounds__(64) void k_aggregate_xent_bwd(const float* __restrict__ samples, const int64_t* __restrict__ labels, float* __restrict__ P,
                                                           float* __restrict__ loss, float* __restrict__ dsamples, int S, int B, float temperature) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.f;
    auto probs_of = [&](int s, float (&p)[C], float (&d)[C]) {
        const float* y = samples + ((size_t)s * B + b) * C;
        float lg[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            d[c] = y[c] - 1.0f;
            lg[c] = d[c] * d[c] * (-1.0f) / temperature;
        }
        float mx = lg[0];
#pragma unroll
        for (int c = 1; c < C; ++c) mx = fmaxf(mx, lg[c]);
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) { lg[c] = expf(lg[c] - mx); sum += lg[c]; }
#pragma unroll
        for (int c = 0; c < C; ++c) p[c] = lg[c] / sum;
    };
    for (int s = 0; s < S; ++s) {
        float p[C], d[C];
        probs_of(s, p, d);
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] += p[c];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) P[(size_t)b * C + c] = acc[c] / (float)S;
    if (!labels) return;
    const int64_t y = labels[b];
    const bool valid = y >= 0 && y < C;
    float Sy = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) Sy = c == y ? acc[c] : Sy;
    loss[b] = valid ? -logf(Sy / (float)S) : NAN;
    const bool live = valid && Sy != 0.f;                  // Sy == 0: loss = +inf above, no gradient; Sy NaN: NaN everywhere
    for (int s = 0; s < S; ++s) {
        float p[C], d[C];
        probs_of(s, p, d);
        float py = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) py = c == y ? p[c] : py;
        const float w = py / Sy;
        float* o = dsamples + ((size_t)s * B + b) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float t = p[c] - (c == y ? 1.0f : 0.0f);
            o[c] = live ? (w * t) * (d[c] * (-2.0f) / temperature) : 0.f;
        }
    }
}

template <int C>
void eg_launch_aggregate(int want, hipStream_t st, const float* samples, const int64_t* labels, float* P, float* loss, float* ds, int S, int B, float temp) {
    if constexpr (C <= EG_MAX_C) {
        if (want == C) hipLaunchKernelGGL(k_aggregate_xent_bwd<C>, dim3((B + 63) / 64), dim3(64), 0, st, samples, labels, P, loss, ds, S, B, temp);
        else eg_launch_aggregate<C + 1>(want, st, samples, labels, P, loss, ds, S, B, temp);
    }
}

// One thread per row of [rows, C]: dot = sum_c dp[c] p[c] in class order, then dlogits[c] = p[c] (dp[c] - dot).
__global__ __launch_bounds__(128) void k_softmax_bwd(const float* __restrict__ p, const float* __restrict__ dp, float* __restrict__ dlogits, int rows, int C) {
#pragma clang fp contract(off)
    const int r = blockIdx.x * 128 + threadIdx.x;
    if (r >= rows) return;
    const float* pr = p + (size_t)r * C;
    const float* dr = dp + (size_t)r * C;
    float dot = 0.f;
    for (int c = 0; c < C; ++c) dot = dot + dr[c] * pr[c];
    for (int c = 0; c < C; ++c) dlogits[(size_t)r * C + c] = pr[c] * (dr[c] - dot);
}

int eg_rows(const char* who, int M, int N, int B) {
    if (M < 1 || B < 1 || M % B || N < 1)
        return nd_set_err(ND_ERR_ARG, "%s needs M >= 1, B >= 1, M %% B == 0 and N >= 1 (M=%d, B=%d, N=%d)", who, M, B, N);
    if (B > 65535) return nd_set_err(ND_ERR_ARG, "%s takes B <= 65535 images (B=%d)", who, B);
    return ND_OK;
}

}  // namespace

extern "C" int nd_cond_mul(const float* s, const float* mul, float* y, int M, int N, int B, void* stream) {
    if (!s || !mul || !y) return nd_set_err(ND_ERR_ARG, "cond_mul: NULL tensor");
    if (int rc = eg_rows("cond_mul", M, N, B)) return rc;
    if (y == mul) return nd_set_err(ND_ERR_ARG, "cond_mul: y must not be mul");
    hipLaunchKernelGGL(k_cond_mul, dim3((unsigned)((N + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, s, mul, y, M, N, B);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_cond_act_bwd(const float* dh, const float* h, const float* a_t, const float* mul, float* du, float* dmul_acc, int M, int N, int B,
                               void* stream) {
    if (!dh || !a_t || !du) return nd_set_err(ND_ERR_ARG, "cond_act_bwd: NULL tensor");
    if (int rc = eg_rows("cond_act_bwd", M, N, B)) return rc;
    if (mul && (!dmul_acc || !h)) return nd_set_err(ND_ERR_ARG, "cond_act_bwd: mul needs dmul_acc and the taped h");
    if (!mul && dmul_acc) return nd_set_err(ND_ERR_ARG, "cond_act_bwd: dmul_acc without mul");
    if (du == h || du == a_t || du == mul || du == dmul_acc || (dmul_acc && (dmul_acc == dh || dmul_acc == h || dmul_acc == a_t || dmul_acc == mul)))
        return nd_set_err(ND_ERR_ARG, "cond_act_bwd: du may alias dh only; dmul_acc aliases nothing");
    hipLaunchKernelGGL(k_cond_act_bwd, dim3((unsigned)((N + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, dh, h, a_t, mul, du,
                       dmul_acc, M, N, B);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_reverse_step(int mode, const float* y, int ldy, const float* ymean, const float* eps, const float* z, float* out, int ldo, int M,
                               int B, int C, float alpha_t, float s_t, float s_tm1, void* stream) {
    if (mode != ND_RSTEP_INIT && mode != ND_RSTEP_UPDATE && mode != ND_RSTEP_LAST) return nd_set_err(ND_ERR_ARG, "reverse_step: unknown mode %d", mode);
    if (!ymean || !out) return nd_set_err(ND_ERR_ARG, "reverse_step: NULL tensor");
    if (mode != ND_RSTEP_LAST && !z) return nd_set_err(ND_ERR_ARG, "reverse_step: this mode needs the draw z");
    if (mode != ND_RSTEP_INIT && (!y || !eps)) return nd_set_err(ND_ERR_ARG, "reverse_step: this mode needs y and eps");
    if (M < 1 || B < 1 || M % B || M > ND_LINEAR_BWD_MAX_M * 64 || C < 1 || C > ND_MAX_C)
        return nd_set_err(ND_ERR_ARG, "reverse_step needs 1 <= M <= %d, B >= 1, M %% B == 0 and 1 <= C <= %d (M=%d, B=%d, C=%d)",
                          ND_LINEAR_BWD_MAX_M * 64, ND_MAX_C, M, B, C);
    if (ldo != C && (ldo < 2 * C || ldo > 64)) return nd_set_err(ND_ERR_ARG, "reverse_step: ldo must be C or in [2C, 64] (ldo=%d, C=%d)", ldo, C);
    if (mode != ND_RSTEP_INIT && (ldy < C || ldy > 64)) return nd_set_err(ND_ERR_ARG, "reverse_step: ldy must lie in [C, 64] (ldy=%d, C=%d)", ldy, C);
    if (out == y || out == ymean || out == eps || out == z) return nd_set_err(ND_ERR_ARG, "reverse_step: out aliases an input");
    hipLaunchKernelGGL(k_reverse_step, dim3((unsigned)((M * ldo + 255) / 256)), dim3(256), 0, (hipStream_t)stream, mode, y, ldy, ymean, eps, z, out,
                       ldo, M, B, C, alpha_t, s_t, s_tm1);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_reverse_step_coef(const float* y, int ldy, const float* ymean, const float* eps, const float* z, float* out, int ldo, int M, int B,
                                    int C, float cy, float cm, float ce, float cz, void* stream) {
    if (!y || !ymean || !eps || !out) return nd_set_err(ND_ERR_ARG, "reverse_step_coef: NULL tensor");
    if (!std::isfinite(cy) || !std::isfinite(cm) || !std::isfinite(ce) || !std::isfinite(cz))
        return nd_set_err(ND_ERR_ARG, "reverse_step_coef: a coefficient is not finite");
    if (!z && cz != 0.f) return nd_set_err(ND_ERR_ARG, "reverse_step_coef: cz=%g needs the draw z", (double)cz);
    if (M < 1 || B < 1 || M % B || M > ND_LINEAR_BWD_MAX_M * 64 || C < 1 || C > ND_MAX_C)
        return nd_set_err(ND_ERR_ARG, "reverse_step_coef needs 1 <= M <= %d, B >= 1, M %% B == 0 and 1 <= C <= %d (M=%d, B=%d, C=%d)",
                          ND_LINEAR_BWD_MAX_M * 64, ND_MAX_C, M, B, C);
    if (ldo != C && (ldo < 2 * C || ldo > 64)) return nd_set_err(ND_ERR_ARG, "reverse_step_coef: ldo must be C or in [2C, 64] (ldo=%d, C=%d)", ldo, C);
    if (ldy < C || ldy > 64) return nd_set_err(ND_ERR_ARG, "reverse_step_coef: ldy must lie in [C, 64] (ldy=%d, C=%d)", ldy, C);
    if (out == y || out == ymean || out == eps || out == z) return nd_set_err(ND_ERR_ARG, "reverse_step_coef: out aliases an input");
    hipLaunchKernelGGL(k_reverse_step_coef, dim3((unsigned)((M * ldo + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y, ldy, ymean, eps, z, out,
                       ldo, M, B, C, cy, cm, ce, cz);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_reverse_step_bwd(const float* g, int ldg, float cy, float cm, float ce, float* deps, float* dyadd, int lda, float* dymean, int M,
                                   int B, int C, void* stream) {
    if (!g || !dymean) return nd_set_err(ND_ERR_ARG, "reverse_step_bwd: NULL tensor");
    if (M < 1 || B < 1 || M % B || M > ND_LINEAR_BWD_MAX_M * 64 || C < 1 || C > ND_MAX_C)
        return nd_set_err(ND_ERR_ARG, "reverse_step_bwd needs 1 <= M <= %d, B >= 1, M %% B == 0 and 1 <= C <= %d (M=%d, B=%d, C=%d)",
                          ND_LINEAR_BWD_MAX_M * 64, ND_MAX_C, M, B, C);
    if (ldg != C && (ldg < 2 * C || ldg > 64)) return nd_set_err(ND_ERR_ARG, "reverse_step_bwd: ldg must be C or in [2C, 64] (ldg=%d, C=%d)", ldg, C);
    if (dyadd && (lda < C || lda > 64)) return nd_set_err(ND_ERR_ARG, "reverse_step_bwd: lda must lie in [C, 64] (lda=%d, C=%d)", lda, C);
    const void* bufs[4] = {g, deps, dyadd, dymean};
    if (nd_any_equal(bufs, 4)) return nd_set_err(ND_ERR_ARG, "reverse_step_bwd: g, deps, dyadd and dymean must be distinct buffers");
    hipLaunchKernelGGL(k_reverse_step_bwd, dim3((unsigned)((B * C + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g, ldg, cy, cm, ce, deps, dyadd,
                       lda, dymean, M, B, C);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_aggregate_xent_bwd(const float* samples, const int64_t* labels, float* P, float* loss, float* dsamples, int S, int B, int C,
                                     float temperature, void* stream) {
    if (!samples || !P) return nd_set_err(ND_ERR_ARG, "aggregate_xent_bwd: NULL tensor");
    if (labels && (!loss || !dsamples)) return nd_set_err(ND_ERR_ARG, "aggregate_xent_bwd: labels need loss and dsamples");
    if (S < 1 || B < 1 || C < 1 || C > EG_MAX_C)
        return nd_set_err(ND_ERR_ARG, "aggregate_xent_bwd needs S, B >= 1 and 1 <= C <= %d (S=%d, B=%d, C=%d)", EG_MAX_C, S, B, C);
    if (!(temperature > 0.f)) return nd_set_err(ND_ERR_ARG, "temperature must be > 0 (temperature=%g)", (double)temperature);
    if (dsamples == samples) return nd_set_err(ND_ERR_ARG, "aggregate_xent_bwd: dsamples must not be samples (they are read twice)");
    eg_launch_aggregate<1>(C, (hipStream_t)stream, samples, labels, P, loss, dsamples, S, B, temperature);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_softmax_bwd(const float* p, const float* dp, float* dlogits, int rows, int C, void* stream) {
    if (!p || !dp || !dlogits) return nd_set_err(ND_ERR_ARG, "softmax_bwd: NULL tensor");
    if (rows < 1 || C < 1) return nd_set_err(ND_ERR_ARG, "softmax_bwd needs rows, C >= 1 (rows=%d, C=%d)", rows, C);
    if (dlogits == p || dlogits == dp) return nd_set_err(ND_ERR_ARG, "softmax_bwd: dlogits must not be an input (a row is read twice)");
    hipLaunchKernelGGL(k_softmax_bwd, dim3((unsigned)((rows + 127) / 128)), dim3(128), 0, (hipStream_t)stream, p, dp, dlogits, rows, C);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}
