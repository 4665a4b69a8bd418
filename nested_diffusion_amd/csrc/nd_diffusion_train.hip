// nd_diffusion_train.hip -- training of the noise estimators (include/nested_diffusion.h: nd_bn_train_fwd, nd_bn_train_bwd, nd_qsample,
// nd_mse_grad, nd_sumsq, nd_clip_adam, nd_clip_adam_ema; the loop: nested_diffusion_amd/train_diffusion.py NoiseEstimatorTrainer).  gfx950 only, fp32 data.
//   k_bn_fwd / k_bn_bwd   BatchNorm1d in training mode fused with ConditionalLinear's per-timestep gain, the softplus and the product with
//                         xe.  A batch has at most 128 rows, so ONE THREAD owns a column and walks its rows in order: the loads of a wave
//                         are 64 adjacent floats of a row (coalesced), no cross-thread reduction exists, and the dense gradient of the
//                         embedding table is summed by the column's owner in row order -- no atomics, the same bits on every run.
//                         A column's statistics and sums are carried in DOUBLE and rounded to fp32 once where they are stored: with two
//                         rows that nearly coincide rstd reaches 1 / sqrt(eps) = 316 and the backward's dz - mean(dz) - xhat mean(dz xhat)
//                         cancels to a few percent of its terms, so an fp32 chain (rstd and xhat off by two ulp) gave du errors twelve
//                         times those of torch's CPU BatchNorm, which accumulates float data in double as well.
//   k_qsample / k_mse     the forward noising with host-gathered per-row coefficients, and the loss with its gradient
//   k_sumsq_*             sum of squares in two stages through a caller workspace, in an order that depends on n alone
//   k_clip_adam           clip coefficient from the summed squares, then nd_optim.hpp's Adam listing, elementwise; its EMA instantiations
//                         end with nd_optim.hpp's shadow update on the new weight, in the same pass
// Bounds: every index below is r * N + n with r < M, n < N, or tr * N + n with 0 <= tr < rows_table checked in the kernel (a row whose
// timestep is outside the table reads and writes no table row), or i < n.
#include "nd_math.hpp"
#include "nd_host.hpp"
#include "nd_optim.hpp"

// every documented line of the fp32 listings (qsample, mse, sumsq, clip + Adam) is one rounded fp32 operation in the listed order (as in
// nd_mlp_train.hip); the BatchNorm kernels' double expressions are not contracted either
#pragma clang fp contract(off)

namespace {

constexpr int BN_THREADS = 64;                   // one wave per workgroup: N = 4096 columns still make 64 workgroups
constexpr int SS_THREADS = 256;
constexpr int SS_PER_THREAD = ND_SUMSQ_CHUNK / SS_THREADS;

// v of row r at column n, as torch forms it: the fp32 product table[t[r]][n] * u[r][n] (u itself without a table); the gain is 0 for a
// timestep outside the table, whose row is then neither read nor written (tr < 0 says so)
__device__ __forceinline__ float bn_v(const float* __restrict__ u, const float* __restrict__ table, const int* __restrict__ t, int rows_table,
                                      int r, int N, int n, float& g, int& tr) {
    const float uv = u[(size_t)r * N + n];
    if (!table) {
        g = 1.f;
        tr = -1;
        return uv;
    }
    tr = t[r];
    if (tr < 0 || tr >= rows_table) {
        g = 0.f;
        tr = -1;
        return 0.f;
    }
    g = table[(size_t)tr * N + n];
    return g * uv;
}

// z = xhat * gamma + beta in double, rounded once: the forward and the backward feed the same float to the activation
__device__ __forceinline__ float bn_z(float xh, float ga, float be) { return (float)((double)xh * (double)ga + (double)be); }

__global__ __launch_bounds__(BN_THREADS) void k_bn_fwd(const float* __restrict__ u, const float* __restrict__ table, const int* __restrict__ t,
                                                       int rows_table, const float* __restrict__ mul, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, float* __restrict__ out, float* __restrict__ xhat,
                                                       float* __restrict__ rstd_out, float* __restrict__ rm, float* __restrict__ rv, int M, int N,
                                                       int act, float eps, float mom) {
    const int n = (int)blockIdx.x * BN_THREADS + (int)threadIdx.x;
    if (n >= N) return;
    const double dM = (double)M;
    float g;
    int tr;
    double s = 0.0;
    for (int r = 0; r < M; ++r) s += (double)bn_v(u, table, t, rows_table, r, N, n, g, tr);
    const double mean = s / dM;
    double q = 0.0;
    for (int r = 0; r < M; ++r) {
        const double d = (double)bn_v(u, table, t, rows_table, r, N, n, g, tr) - mean;
        q += d * d;
    }
    const double var = q / dM;
    const double rstd = 1.0 / sqrt(var + (double)eps);
    const float ga = gamma[n], be = beta[n];
    for (int r = 0; r < M; ++r) {
        const size_t i = (size_t)r * N + n;
        const float xh = (float)(((double)bn_v(u, table, t, rows_table, r, N, n, g, tr) - mean) * rstd);
        const float z = bn_z(xh, ga, be);
        const float a = act == ND_ACT_SOFTPLUS ? nd_softplus(z) : z;
        xhat[i] = xh;
        out[i] = mul ? a * mul[i] : a;
    }
    rstd_out[n] = (float)rstd;
    if (rm) rm[n] = (float)((1.0 - (double)mom) * (double)rm[n] + (double)mom * mean);
    if (rv) rv[n] = (float)((1.0 - (double)mom) * (double)rv[n] + (double)mom * (var * (dM / (dM - 1.0))));
}

// dz of one element: da through the activation at z
__device__ __forceinline__ double bn_dz(double da, float z, int act) {
    if (act != ND_ACT_SOFTPLUS || z > 20.0f) return da;
    return da * (1.0 / (1.0 + exp(-(double)z)));
}

__global__ __launch_bounds__(BN_THREADS) void k_bn_bwd(const float* __restrict__ dout, const float* __restrict__ u, const float* __restrict__ table,
                                                       const int* __restrict__ t, int rows_table, const float* __restrict__ mul,
                                                       const float* __restrict__ xhat, const float* __restrict__ rstd_in,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ du,
                                                       float* __restrict__ dmul, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                       float* __restrict__ dtable, int M, int N, int act) {
    const int n = (int)blockIdx.x * BN_THREADS + (int)threadIdx.x;
    if (n >= N) return;
    const double dM = (double)M;
    const float ga = gamma[n], be = beta[n];
    double dg = 0.0, db = 0.0;
    for (int r = 0; r < M; ++r) {
        const size_t i = (size_t)r * N + n;
        const float xh = xhat[i], d = dout[i];
        const float z = bn_z(xh, ga, be);
        if (dmul) dmul[i] = d * (act == ND_ACT_SOFTPLUS ? nd_softplus(z) : z);
        const double dz = bn_dz(mul ? (double)d * (double)mul[i] : (double)d, z, act);
        dg += dz * (double)xh;
        db += dz;
    }
    dgamma[n] = (float)dg;
    dbeta[n] = (float)db;
    const double k = (double)ga * (double)rstd_in[n], mb = db / dM, mg = dg / dM;
    for (int r = 0; r < M; ++r) {
        const size_t i = (size_t)r * N + n;
        const float xh = xhat[i], d = dout[i];
        const double dz = bn_dz(mul ? (double)d * (double)mul[i] : (double)d, bn_z(xh, ga, be), act);
        const double dv = k * ((dz - mb) - ((double)xh * mg));
        if (table) {
            float g;
            int tr;
            bn_v(u, table, t, rows_table, r, N, n, g, tr);
            if (tr >= 0) {
                const size_t j = (size_t)tr * N + n;        // this thread is the only writer of column n: a plain read-modify-write
                dtable[j] = (float)((double)dtable[j] + dv * (double)u[i]);
            }
            du[i] = (float)(dv * (double)g);
        } else {
            du[i] = (float)dv;
        }
    }
}

__global__ __launch_bounds__(256) void k_qsample(const float* __restrict__ y0, const float* __restrict__ yhat, const float* __restrict__ e,
                                                 const float* __restrict__ ca, const float* __restrict__ cb, float* __restrict__ yt, int M, int C) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= M * C) return;
    const int r = i / C;
    const float a = ca[r];
    yt[i] = ((a * y0[i]) + ((1.0f - a) * yhat[i])) + (cb[r] * e[i]);
}

// one workgroup: the gradient elementwise, the loss by thread 0 in row-major order
__global__ __launch_bounds__(256) void k_mse(const float* __restrict__ out, const float* __restrict__ e, float* __restrict__ dout,
                                             float* __restrict__ loss, int n, float gscale) {
    for (int i = (int)threadIdx.x; i < n; i += 256) dout[i] = (out[i] - e[i]) * gscale;
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int i = 0; i < n; ++i) {
            const float d = e[i] - out[i];
            s += d * d;
        }
        loss[0] = s / (float)n;
    }
}

// the tree both stages end with: 256 values in LDS, s[j] += s[j + h] for h = 128, 64 .. 1
__device__ __forceinline__ float ss_tree(float p, float* s) {
    const int j = (int)threadIdx.x;
    s[j] = p;
    __syncthreads();
    for (int h = SS_THREADS / 2; h > 0; h >>= 1) {
        if (j < h) s[j] = s[j] + s[j + h];
        __syncthreads();
    }
    return s[0];
}

__global__ __launch_bounds__(SS_THREADS) void k_sumsq_chunks(const float* __restrict__ x, float* __restrict__ part, size_t n) {
    __shared__ float s[SS_THREADS];
    const size_t base = (size_t)blockIdx.x * ND_SUMSQ_CHUNK + threadIdx.x;
    float p = 0.f;
#pragma unroll
    for (int i = 0; i < SS_PER_THREAD; ++i) {
        const size_t k = base + (size_t)i * SS_THREADS;
        if (k < n) {
            const float v = x[k];
            p += v * v;
        }
    }
    const float tot = ss_tree(p, s);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

__global__ __launch_bounds__(SS_THREADS) void k_sumsq_final(const float* __restrict__ part, float* __restrict__ acc, size_t chunks, int accumulate) {
    __shared__ float s[SS_THREADS];
    float p = 0.f;
    for (size_t c = threadIdx.x; c < chunks; c += SS_THREADS) p += part[c];
    const float tot = ss_tree(p, s);
    if (threadIdx.x == 0) acc[0] = accumulate ? acc[0] + tot : tot;
}

__device__ __forceinline__ float clip_coef(const float* sumsq, float max_norm) {
    if (!sumsq) return 1.0f;
    const float total = sqrtf(sumsq[0]);
    const float c = max_norm / (total + 1e-6f);
    return (c < 1.0f) ? c : 1.0f;
}

// EMA: the shadow s rides in the same pass (nd_clip_adam_ema): one more load and one more store per element, no second read of w
template <bool VEC, bool EMA>
__global__ __launch_bounds__(256) void k_clip_adam(float* __restrict__ w, float* __restrict__ m, float* __restrict__ v, const float* __restrict__ g,
                                                   float* __restrict__ s, size_t n, const float* __restrict__ sumsq, float max_norm, int clip,
                                                   nd_adam_step a, nd_ema_step e) {
    const float coef = clip_coef(clip ? sumsq : nullptr, max_norm);
    const size_t stride = (size_t)gridDim.x * 256;
    if (VEC) {                                      // n % 4 == 0 and 16-byte aligned tensors
        const size_t n4 = n / 4;
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
            float4 w4 = reinterpret_cast<float4*>(w)[i], m4 = reinterpret_cast<float4*>(m)[i], v4 = reinterpret_cast<float4*>(v)[i];
            const float4 g4 = reinterpret_cast<const float4*>(g)[i];
            float4 s4;
            if (EMA) s4 = reinterpret_cast<float4*>(s)[i];
            const float gx = clip ? g4.x * coef : g4.x, gy = clip ? g4.y * coef : g4.y, gz = clip ? g4.z * coef : g4.z,
                        gw = clip ? g4.w * coef : g4.w;
            nd_optim_update(w4.x, m4.x, v4.x, gx, a);
            nd_optim_update(w4.y, m4.y, v4.y, gy, a);
            nd_optim_update(w4.z, m4.z, v4.z, gz, a);
            nd_optim_update(w4.w, m4.w, v4.w, gw, a);
            reinterpret_cast<float4*>(w)[i] = w4;
            reinterpret_cast<float4*>(m)[i] = m4;
            reinterpret_cast<float4*>(v)[i] = v4;
            if (EMA) {
                nd_ema_update(s4.x, w4.x, e);
                nd_ema_update(s4.y, w4.y, e);
                nd_ema_update(s4.z, w4.z, e);
                nd_ema_update(s4.w, w4.w, e);
                reinterpret_cast<float4*>(s)[i] = s4;
            }
        }
    } else {
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
            float wv = w[i], mv = m[i], vv = v[i];
            const float gv = clip ? g[i] * coef : g[i];
            nd_optim_update(wv, mv, vv, gv, a);
            w[i] = wv;
            m[i] = mv;
            v[i] = vv;
            if (EMA) {
                float sv = s[i];
                nd_ema_update(sv, wv, e);
                s[i] = sv;
            }
        }
    }
}

int bn_shape_check(const char* what, int M, int N, int act, const void* table, const void* t, int rows_table) {
    if (M < 2 || M > ND_LINEAR_BWD_MAX_M)
        return nd_set_err(ND_ERR_ARG, "%s needs 2 <= M <= %d (M=%d): batch statistics need two rows", what, ND_LINEAR_BWD_MAX_M, M);
    if (N < 1) return nd_set_err(ND_ERR_ARG, "%s needs N >= 1 (N=%d)", what, N);
    if ((size_t)M * (size_t)N > (size_t)INT32_MAX) return nd_set_err(ND_ERR_ARG, "%s: M * N does not fit an int (M=%d, N=%d)", what, M, N);
    if (act != ND_ACT_NONE && act != ND_ACT_SOFTPLUS) return nd_set_err(ND_ERR_ARG, "%s: act must be ND_ACT_NONE or ND_ACT_SOFTPLUS (act=%d)", what, act);
    if ((table != nullptr) != (t != nullptr)) return nd_set_err(ND_ERR_ARG, "%s: table and t come together", what);
    if (table && rows_table < 1) return nd_set_err(ND_ERR_ARG, "%s needs rows_table >= 1 (rows_table=%d)", what, rows_table);
    return ND_OK;
}

}  // namespace

extern "C" int nd_bn_train_fwd(const float* u, const float* table, const int32_t* t, int rows_table, const float* mul, const float* gamma,
                               const float* beta, float* out, float* xhat, float* rstd, float* running_mean, float* running_var, int M, int N,
                               int act, float eps, float momentum, void* stream) {
    if (!u || !gamma || !beta || !out || !xhat || !rstd) return nd_set_err(ND_ERR_ARG, "bn_train_fwd: NULL tensor");
    if (const int rc = bn_shape_check("bn_train_fwd", M, N, act, table, t, rows_table)) return rc;
    if (!(eps >= 0.f)) return nd_set_err(ND_ERR_ARG, "bn_train_fwd needs eps >= 0");
    if (nd_misaligned(u, 3) || nd_misaligned(table, 3) || nd_misaligned(t, 3) || nd_misaligned(mul, 3) || nd_misaligned(gamma, 3) ||
        nd_misaligned(beta, 3) || nd_misaligned(out, 3) || nd_misaligned(xhat, 3) || nd_misaligned(rstd, 3) || nd_misaligned(running_mean, 3) ||
        nd_misaligned(running_var, 3))
        return nd_set_err(ND_ERR_ARG, "bn_train_fwd: misaligned tensor");
    const void* outs[5] = {out, xhat, rstd, running_mean, running_var};
    if (nd_any_equal(outs, 5) || out == u || xhat == u || out == mul || xhat == mul)
        return nd_set_err(ND_ERR_ARG, "bn_train_fwd: the outputs must be distinct buffers, and none of them an input");
    hipLaunchKernelGGL(k_bn_fwd, dim3((unsigned)((N + BN_THREADS - 1) / BN_THREADS)), dim3(BN_THREADS), 0, (hipStream_t)stream, u, table,
                       (const int*)t, rows_table, mul, gamma, beta, out, xhat, rstd, running_mean, running_var, M, N, act, eps, momentum);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_bn_train_bwd(const float* dout, const float* u, const float* table, const int32_t* t, int rows_table, const float* mul,
                               const float* xhat, const float* rstd, const float* gamma, const float* beta, float* du, float* dmul,
                               float* dgamma, float* dbeta, float* dtable, int M, int N, int act, void* stream) {
    if (!dout || !xhat || !rstd || !gamma || !beta || !du || !dgamma || !dbeta) return nd_set_err(ND_ERR_ARG, "bn_train_bwd: NULL tensor");
    if (const int rc = bn_shape_check("bn_train_bwd", M, N, act, table, t, rows_table)) return rc;
    if (table && (!u || !dtable)) return nd_set_err(ND_ERR_ARG, "bn_train_bwd: the gain needs u and dtable");
    if (dmul && !mul) return nd_set_err(ND_ERR_ARG, "bn_train_bwd: dmul without mul");
    if (nd_misaligned(dout, 3) || nd_misaligned(u, 3) || nd_misaligned(table, 3) || nd_misaligned(t, 3) || nd_misaligned(mul, 3) ||
        nd_misaligned(xhat, 3) || nd_misaligned(rstd, 3) || nd_misaligned(gamma, 3) || nd_misaligned(beta, 3) || nd_misaligned(du, 3) ||
        nd_misaligned(dmul, 3) || nd_misaligned(dgamma, 3) || nd_misaligned(dbeta, 3) || nd_misaligned(dtable, 3))
        return nd_set_err(ND_ERR_ARG, "bn_train_bwd: misaligned tensor");
    const void* outs[5] = {du, dmul, dgamma, dbeta, dtable};
    const void* ins[7] = {dout, u, table, mul, xhat, gamma, beta};
    bool alias = nd_any_equal(outs, 5);
    for (int i = 0; i < 5; ++i)
        for (int j = 0; j < 7; ++j) alias = alias || (outs[i] && outs[i] == ins[j]);
    if (alias) return nd_set_err(ND_ERR_ARG, "bn_train_bwd: the outputs must be distinct buffers, and none of them an input");
    hipStream_t st = (hipStream_t)stream;
    if (table) HIP_CHECK(hipMemsetAsync(dtable, 0, (size_t)rows_table * (size_t)N * sizeof(float), st));
    hipLaunchKernelGGL(k_bn_bwd, dim3((unsigned)((N + BN_THREADS - 1) / BN_THREADS)), dim3(BN_THREADS), 0, st, dout, u, table, (const int*)t,
                       rows_table, mul, xhat, rstd, gamma, beta, du, dmul, dgamma, dbeta, dtable, M, N, act);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_qsample(const float* y0, const float* yhat, const float* e, const float* ca, const float* cb, float* yt, int M, int C,
                          void* stream) {
    if (!y0 || !yhat || !e || !ca || !cb || !yt) return nd_set_err(ND_ERR_ARG, "qsample: NULL tensor");
    if (M < 1 || M > ND_LINEAR_BWD_MAX_M || C < 1 || C > ND_MSE_MAX_C)
        return nd_set_err(ND_ERR_ARG, "qsample needs 1 <= M <= %d and 1 <= C <= %d (M=%d, C=%d)", ND_LINEAR_BWD_MAX_M, ND_MSE_MAX_C, M, C);
    if (nd_misaligned(y0, 3) || nd_misaligned(yhat, 3) || nd_misaligned(e, 3) || nd_misaligned(ca, 3) || nd_misaligned(cb, 3) || nd_misaligned(yt, 3))
        return nd_set_err(ND_ERR_ARG, "qsample: misaligned tensor");
    hipLaunchKernelGGL(k_qsample, dim3((unsigned)((M * C + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y0, yhat, e, ca, cb, yt, M, C);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_mse_grad(const float* out, const float* e, float* dout, float* loss, int M, int C, void* stream) {
    if (!out || !e || !dout || !loss) return nd_set_err(ND_ERR_ARG, "mse_grad: NULL tensor");
    if (M < 1 || M > ND_LINEAR_BWD_MAX_M || C < 1 || C > ND_MSE_MAX_C)
        return nd_set_err(ND_ERR_ARG, "mse_grad needs 1 <= M <= %d and 1 <= C <= %d (M=%d, C=%d)", ND_LINEAR_BWD_MAX_M, ND_MSE_MAX_C, M, C);
    if (nd_misaligned(out, 3) || nd_misaligned(e, 3) || nd_misaligned(dout, 3) || nd_misaligned(loss, 3))
        return nd_set_err(ND_ERR_ARG, "mse_grad: misaligned tensor");
    if (dout == out || dout == e) return nd_set_err(ND_ERR_ARG, "mse_grad: dout must not alias an input (the loss reads them after it is written)");
    const int n = M * C;
    hipLaunchKernelGGL(k_mse, dim3(1), dim3(256), 0, (hipStream_t)stream, out, e, dout, loss, n, 2.0f / (float)n);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_sumsq_plan(size_t n, size_t* out2) {
    if (!out2) return nd_set_err(ND_ERR_ARG, "sumsq_plan: NULL out");
    if (n < 1 || n > ND_SUMSQ_MAX_N) return nd_set_err(ND_ERR_ARG, "sumsq_plan needs 1 <= n <= 2^40 (n=%zu)", n);
    const size_t chunks = (n + ND_SUMSQ_CHUNK - 1) / ND_SUMSQ_CHUNK;
    out2[0] = chunks;
    // the longest serial chain of additions: a thread's elements, the tree, a thread's partials, the tree, the add to acc
    out2[1] = (size_t)SS_PER_THREAD + 8 + (chunks + SS_THREADS - 1) / SS_THREADS + 8 + 1;
    return ND_OK;
}

extern "C" size_t nd_sumsq_workspace_bytes(size_t n) {
    if (n < 1 || n > ND_SUMSQ_MAX_N) return 0;
    return ((n + ND_SUMSQ_CHUNK - 1) / ND_SUMSQ_CHUNK) * sizeof(float);
}

extern "C" int nd_sumsq(const float* x, size_t n, float* acc, int accumulate, void* ws, size_t ws_bytes, void* stream) {
    if (!x || !acc) return nd_set_err(ND_ERR_ARG, "sumsq: NULL tensor");
    const size_t need = nd_sumsq_workspace_bytes(n);
    if (!need) return nd_set_err(ND_ERR_ARG, "sumsq needs 1 <= n <= 2^40 (n=%zu)", n);
    if (!ws || ws_bytes < need) return nd_set_err(ND_ERR_ARG, "sumsq: workspace too small: %zu < %zu", ws_bytes, need);
    if (nd_misaligned(x, 3) || nd_misaligned(acc, 3) || nd_misaligned(ws, 3)) return nd_set_err(ND_ERR_ARG, "sumsq: misaligned tensor");
    const size_t chunks = need / sizeof(float);
    if (chunks > (size_t)INT32_MAX) return nd_set_err(ND_ERR_ARG, "sumsq: too many chunks");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_sumsq_chunks, dim3((unsigned)chunks), dim3(SS_THREADS), 0, st, x, (float*)ws, n);
    hipLaunchKernelGGL(k_sumsq_final, dim3(1), dim3(SS_THREADS), 0, st, (const float*)ws, acc, chunks, accumulate ? 1 : 0);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

// the checks and the launch nd_clip_adam and nd_clip_adam_ema share; s and e NULL: no shadow (what: the entry point's name in a refusal)
static int clip_adam_launch(const char* what, float* w, float* m, float* v, const float* g, float* s, size_t n, const float* sumsq, float max_norm,
                            const nd_adam_step* a, const nd_ema_step* e, void* stream) {
    const bool ema = e != nullptr;
    if (!w || !m || !v || !g || !a || (ema && !s)) return nd_set_err(ND_ERR_ARG, "%s: NULL tensor", what);
    if (n < 1) return nd_set_err(ND_ERR_ARG, "%s needs n >= 1", what);
    if (nd_misaligned(w, 3) || nd_misaligned(m, 3) || nd_misaligned(v, 3) || nd_misaligned(g, 3) || nd_misaligned(sumsq, 3) ||
        (ema && nd_misaligned(s, 3)))
        return nd_set_err(ND_ERR_ARG, "%s: misaligned tensor", what);
    const void* p[5] = {w, m, v, g, s};
    if (nd_any_equal(p, ema ? 5 : 4)) return nd_set_err(ND_ERR_ARG, "%s: w, m, v%s and g must be distinct buffers", what, ema ? ", s" : "");
    const bool vec = n % 4 == 0 && !nd_misaligned(w, 15) && !nd_misaligned(m, 15) && !nd_misaligned(v, 15) && !nd_misaligned(g, 15) &&
                     !(ema && nd_misaligned(s, 15));
    const unsigned blocks = nd_blocks_per_image(vec ? n / 4 : n, 16384);
    hipStream_t st = (hipStream_t)stream;
    const int clip = sumsq ? 1 : 0;
    const nd_ema_step ev = ema ? *e : nd_ema_step{};
    if (ema) {
        if (vec) hipLaunchKernelGGL((k_clip_adam<true, true>), dim3(blocks), dim3(256), 0, st, w, m, v, g, s, n, sumsq, max_norm, clip, *a, ev);
        else hipLaunchKernelGGL((k_clip_adam<false, true>), dim3(blocks), dim3(256), 0, st, w, m, v, g, s, n, sumsq, max_norm, clip, *a, ev);
    } else {
        if (vec) hipLaunchKernelGGL((k_clip_adam<true, false>), dim3(blocks), dim3(256), 0, st, w, m, v, g, s, n, sumsq, max_norm, clip, *a, ev);
        else hipLaunchKernelGGL((k_clip_adam<false, false>), dim3(blocks), dim3(256), 0, st, w, m, v, g, s, n, sumsq, max_norm, clip, *a, ev);
    }
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_clip_adam(float* w, float* m, float* v, const float* g, size_t n, const float* sumsq, float max_norm, const nd_adam_step* a,
                            void* stream) {
    return clip_adam_launch("clip_adam", w, m, v, g, nullptr, n, sumsq, max_norm, a, nullptr, stream);
}

extern "C" int nd_clip_adam_ema(float* w, float* m, float* v, const float* g, float* s, size_t n, const float* sumsq, float max_norm,
                                const nd_adam_step* a, const nd_ema_step* e, void* stream) {
    if (!s || !e) return nd_set_err(ND_ERR_ARG, "clip_adam_ema: NULL %s", !s ? "shadow s" : "nd_ema_step");
    return clip_adam_launch("clip_adam_ema", w, m, v, g, s, n, sumsq, max_norm, a, e, stream);
}
