// nd_attack_linf.hip -- the Linf attack steps between two ViT passes: what foolbox's LinfBaseGradientDescent (attack.py) and AutoAttack's
// APGD-CE (autoattack.py) do to the image once nd_vit_grad.hip has produced the input gradient.  gfx950 only, all arithmetic fp32.
//   k_linf_step         x0 + clip(x + a sign(g) - x0, -eps, eps), clipped to the bounds (foolbox's order)
//   k_linf_start        x0 + U[-eps, eps) from Philox4x32-10, clipped to the bounds
//   k_apgd_start_max    AutoAttack APGD's random start, pass 1: per-image max |t| of the Philox draws (atomic max on the bit pattern)
//   k_apgd_start        pass 2: x0 + eps * t / (max|t| + 1e-12), the draws recomputed, clipped to the bounds
//   k_apgd_control      APGD's per-image bookkeeping of one iteration: acc, best loss, the checkpoint rule; writes the flags
//   k_apgd_update       APGD's per-element work of one iteration: best / best-adversarial copies, restore, the momentum step
#include "nd_attack.hpp"
#include "nd_philox.hpp"

// Every operation below is a single rounded fp32 op in foolbox's (AutoAttack's) order: contraction is off, and the __f*_rn helpers of the
// HIP headers are not used (their multiply and add fuse into an FMA), so a float32 restatement on the host reproduces them bit for bit.
#pragma clang fp contract(off)

// ---------------------------------------------------------------------------------------------
// Linf steps
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_linf_step(const float* __restrict__ x, const float* __restrict__ x0, const float* __restrict__ g,
                                                   float* __restrict__ out, size_t n, float alpha, float eps, float lo, float hi) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float s = 0.f;
        if (g) s = g[i] > 0.f ? 1.f : (g[i] < 0.f ? -1.f : 0.f);
        const float a = x0[i];
        const float step = x[i] + alpha * s;
        const float d = nd_clampf(step - a, -eps, eps);
        out[i] = nd_clampf(a + d, lo, hi);
    }
}

// one thread per 4 elements of one image (per_image % 4 == 0); see nd_linf_random_start in the header for the mapping
__global__ __launch_bounds__(256) void k_linf_start(const float* __restrict__ x0, float* __restrict__ out, int B, int quads, uint64_t seed,
                                                    uint32_t first_image, uint32_t restart, float eps, float lo, float hi) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)B * quads) return;
    const int b = (int)(idx / quads), q = (int)(idx - (size_t)b * quads);
    uint32_t c[4] = {first_image + (uint32_t)b, (uint32_t)q, restart, ND_LINF_START_TAG};
    nd_philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const size_t o = idx * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float w = 2.0f * nd_u24(c[e]) - 1.0f;                                    // [-1, 1): exact
        out[o + e] = nd_clampf(x0[o + e] + eps * w, lo, hi);                           // two roundings (contraction is off in this file)
    }
}

// ---------------------------------------------------------------------------------------------
// AutoAttack APGD-CE, Linf (autopgd_base.py attack_single_run; the listing is in nested_diffusion_amd/autoattack.py).  Same rules as
// the Linf steps above: every operation one rounded fp32 op in the reference's order.  Grids are (blocks per image, images): every
// workgroup belongs to one image, so the per-image scalars (step, flags, max) are workgroup-uniform.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void nd_apgd_draw(float (&t)[4], uint32_t image, uint32_t q, uint32_t restart, uint64_t seed) {
    uint32_t c[4] = {image, q, restart, ND_APGD_START_TAG};
    nd_philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
    for (int e = 0; e < 4; ++e) t[e] = 2.0f * nd_u24(c[e]) - 1.0f;   // 2u - 1: exact
}

// pass 1: m_ws[b] = bits of max |t| over image b (|t| >= 0: the uint order of the bits is the float order, and a max is exact in any order)
__global__ __launch_bounds__(256) void k_apgd_start_max(const int64_t* __restrict__ index, uint32_t* __restrict__ m_ws, int quads, uint64_t seed,
                                                        uint32_t restart) {
    __shared__ uint32_t part[4];
    const int b = blockIdx.y;
    const uint32_t image = (uint32_t)index[b];
    uint32_t m = 0;
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += gridDim.x * blockDim.x) {
        float t[4];
        nd_apgd_draw(t, image, (uint32_t)q, restart, seed);
#pragma unroll
        for (int e = 0; e < 4; ++e) m = max(m, __float_as_uint(fabsf(t[e])));
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(&m_ws[b], max(max(part[0], part[1]), max(part[2], part[3])));
}

// pass 2: out = clip(x0 + eps * (t / (m + 1e-12)), lo, hi): autoattack's x + eps * normalize(t), then clamp(0, 1)
__global__ __launch_bounds__(256) void k_apgd_start(const float* __restrict__ x0, const int64_t* __restrict__ index, const uint32_t* __restrict__ m_ws,
                                                    float* __restrict__ out, int quads, uint64_t seed, uint32_t restart, float eps, float lo, float hi) {
    const int b = blockIdx.y;
    const uint32_t image = (uint32_t)index[b];
    const float den = __uint_as_float(m_ws[b]) + 1e-12f;
    const float4* xi = reinterpret_cast<const float4*>(x0) + (size_t)b * quads;
    float4* oi = reinterpret_cast<float4*>(out) + (size_t)b * quads;
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += gridDim.x * blockDim.x) {
        float t[4];
        nd_apgd_draw(t, image, (uint32_t)q, restart, seed);
        const float4 v = xi[q];
        float4 r;
        r.x = nd_clampf(v.x + eps * (t[0] / den), lo, hi);
        r.y = nd_clampf(v.y + eps * (t[1] / den), lo, hi);
        r.z = nd_clampf(v.z + eps * (t[2] / den), lo, hi);
        r.w = nd_clampf(v.w + eps * (t[3] / den), lo, hi);
        oi[q] = r;
    }
}

// one thread per image: iter < 0 initialises the state from the start point's logits / loss; else iteration iter, with a checkpoint of
// length k when k > 0 (the host knows the fixed schedule; every decision is made here, so an iteration needs no host synchronisation)
__global__ __launch_bounds__(64) void k_apgd_control(const float* __restrict__ logits, const int64_t* __restrict__ labels, const float* __restrict__ loss,
                                                     float* __restrict__ step, float* __restrict__ loss_best, float* __restrict__ loss_best_last_check,
                                                     int32_t* __restrict__ reduced_last_check, int32_t* __restrict__ acc, float* __restrict__ loss_steps,
                                                     int32_t* __restrict__ flags, int B, int C, int n_iter, int iter, int k, float rho, float step0) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float* l = logits + (size_t)b * C;
    int arg = 0;                                        // argmax: the first maximal index (a NaN logit never wins; all NaN: index 0)
    float best = l[0];
    for (int c = 1; c < C; ++c) {
        const float v = l[c];
        if (v > best || (best != best && v == v)) { best = v; arg = c; }      // a NaN held from column 0 yields to the first number
    }
    const bool pred = (int64_t)arg == labels[b];
    const float lb = loss[b];
    if (iter < 0) {
        acc[b] = pred;
        loss_best[b] = lb;
        loss_best_last_check[b] = lb;
        reduced_last_check[b] = 1;
        step[b] = step0;
        for (int j = 0; j < n_iter; ++j) loss_steps[(size_t)j * B + b] = 0.f;
        flags[b] = 0;
        return;
    }
    acc[b] = acc[b] && pred;
    loss_steps[(size_t)iter * B + b] = lb;
    float best_loss = loss_best[b];
    const bool imp = lb > best_loss;
    if (imp) best_loss = lb;
    loss_best[b] = best_loss;
    bool restore = false;
    if (k > 0) {
        int cnt = 0;                                    // check_oscillation: row -1 is row n_iter - 1 (torch's negative index)
        for (int c = 0; c < k; ++c) {
            const int j = iter - c, jm = j - 1 < 0 ? j - 1 + n_iter : j - 1;
            cnt += loss_steps[(size_t)j * B + b] > loss_steps[(size_t)jm * B + b];
        }
        const bool osc = (float)cnt <= (float)k * rho || (reduced_last_check[b] == 0 && loss_best_last_check[b] >= best_loss);
        reduced_last_check[b] = osc;
        loss_best_last_check[b] = best_loss;
        if (osc) step[b] = step[b] / 2.0f;
        restore = osc;
    }
    flags[b] = (pred ? 0 : ND_APGD_NOT_PRED) | (imp ? ND_APGD_IMPROVED : 0) | (restore ? ND_APGD_RESTORE : 0);
}

// z = clamp(min(max(xa + step * sign(g), x - eps), x + eps), 0, 1);
// new = clamp(min(max(xa + (z - xa) * a + (xa - xold) * (1 - a), x - eps), x + eps), 0, 1)
__device__ __forceinline__ float nd_apgd_step(float xa, float xold, float g, float x, float st, float eps, float a, float one_minus_a) {
    const float s = g > 0.f ? 1.f : (g < 0.f ? -1.f : 0.f);      // sign(NaN) = 0: no step
    const float lo = x - eps, hi = x + eps;
    const float z = nd_clampf(fminf(fmaxf(xa + st * s, lo), hi), 0.f, 1.f);
    const float v = (xa + (z - xa) * a) + (xa - xold) * one_minus_a;
    return nd_clampf(fminf(fmaxf(v, lo), hi), 0.f, 1.f);
}

template <bool APPLY, bool STEP>
__global__ __launch_bounds__(256) void k_apgd_update(const float* __restrict__ x, float* x_adv, float* x_adv_old, const float* __restrict__ grad,
                                                     float* __restrict__ x_best, float* __restrict__ grad_best, float* __restrict__ x_best_adv,
                                                     const int32_t* __restrict__ flags, const float* __restrict__ step, int quads, float eps, float a) {
    const int b = blockIdx.y;
    const int f = APPLY ? flags[b] : 0;
    const float st = STEP ? step[b] : 0.f, one_minus_a = 1.0f - a;
    const size_t base = (size_t)b * quads;
    float4* xa4 = reinterpret_cast<float4*>(x_adv) + base;
    const float4* g4 = reinterpret_cast<const float4*>(grad) + base;
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += gridDim.x * blockDim.x) {
        float4 xa = xa4[q], g = STEP ? g4[q] : float4{};
        if (APPLY) {
            if (f & ND_APGD_NOT_PRED) reinterpret_cast<float4*>(x_best_adv)[base + q] = xa;
            if (f & ND_APGD_IMPROVED) {
                if (!STEP) g = g4[q];
                reinterpret_cast<float4*>(x_best)[base + q] = xa;
                reinterpret_cast<float4*>(grad_best)[base + q] = g;
            }
            if ((f & ND_APGD_RESTORE) && !(f & ND_APGD_IMPROVED)) {    // x_adv = x_best, grad = grad_best (an improvement is already both)
                xa = reinterpret_cast<const float4*>(x_best)[base + q];
                if (STEP) g = reinterpret_cast<const float4*>(grad_best)[base + q];
                else xa4[q] = xa;
            }
        }
        if (STEP) {
            const float4 xo = reinterpret_cast<const float4*>(x_adv_old)[base + q], x0 = reinterpret_cast<const float4*>(x)[base + q];
            reinterpret_cast<float4*>(x_adv_old)[base + q] = xa;
            float4 r;
            r.x = nd_apgd_step(xa.x, xo.x, g.x, x0.x, st, eps, a, one_minus_a);
            r.y = nd_apgd_step(xa.y, xo.y, g.y, x0.y, st, eps, a, one_minus_a);
            r.z = nd_apgd_step(xa.z, xo.z, g.z, x0.z, st, eps, a, one_minus_a);
            r.w = nd_apgd_step(xa.w, xo.w, g.w, x0.w, st, eps, a, one_minus_a);
            xa4[q] = r;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
constexpr size_t LINF_MAX_QUADS = 0x7FFFFFFF;   // quads are an int in every kernel here, and every loop runs to q < quads
constexpr unsigned APGD_MAX_BLOCKS = 1024;  // workgroups per image

extern "C" int nd_linf_step(const float* x, const float* x0, const float* grad, float* out, size_t n, float alpha, float eps, float lo, float hi,
                            void* stream) {
    if (!x || !x0 || !out) return nd_set_err(ND_ERR_ARG, "NULL tensor");
    if (n == 0) return ND_OK;
    hipLaunchKernelGGL(k_linf_step, dim3(nd_blocks_per_image(n, 8192)), dim3(256), 0, (hipStream_t)stream, x, x0, grad, out, n, alpha, eps, lo, hi);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

// (the image is not a grid dimension here: no B <= 65535 limit)
extern "C" int nd_linf_random_start(const float* x0, float* out, int B, size_t per_image, uint64_t seed, uint32_t first_image, uint32_t restart,
                                    float eps, float lo, float hi, void* stream) {
    if (!x0 || !out) return nd_set_err(ND_ERR_ARG, "NULL tensor");
    if (int rc = nd_check_rows("random start", B, per_image, 0x7FFFFFFF, LINF_MAX_QUADS)) return rc;
    const int quads = (int)(per_image / 4);
    const size_t n = (size_t)B * quads;
    hipLaunchKernelGGL(k_linf_start, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x0, out, B, quads, seed, first_image, restart,
                       eps, lo, hi);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_apgd_random_start(const float* x0, const int64_t* index, float* out, uint32_t* m_ws, int B, size_t per_image, uint64_t seed,
                                    uint32_t restart, float eps, float lo, float hi, void* stream) {
    if (!x0 || !index || !out || !m_ws) return nd_set_err(ND_ERR_ARG, "NULL tensor");
    if (int rc = nd_check_rows("apgd random start", B, per_image, 65535, LINF_MAX_QUADS)) return rc;
    if (nd_misaligned(x0, 15) || nd_misaligned(out, 15)) return nd_set_err(ND_ERR_ARG, "apgd random start needs 16-byte aligned images");
    const int quads = (int)(per_image / 4);
    const dim3 grid = nd_image_grid(B, quads, APGD_MAX_BLOCKS);
    hipStream_t st = (hipStream_t)stream;
    HIP_CHECK(hipMemsetAsync(m_ws, 0, (size_t)B * sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_apgd_start_max, grid, dim3(256), 0, st, index, m_ws, quads, seed, restart);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_apgd_start, grid, dim3(256), 0, st, x0, index, m_ws, out, quads, seed, restart, eps, lo, hi);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_apgd_control(const float* logits, const int64_t* labels, const float* loss, float* step, float* loss_best,
                               float* loss_best_last_check, int32_t* reduced_last_check, int32_t* acc, float* loss_steps, int32_t* flags, int B,
                               int C, int n_iter, int iter, int k, float rho, float step0, void* stream) {
    if (!logits || !labels || !loss || !step || !loss_best || !loss_best_last_check || !reduced_last_check || !acc || !loss_steps || !flags)
        return nd_set_err(ND_ERR_ARG, "NULL tensor");
    if (B < 1 || C < 1 || C > 1024 || n_iter < 1) return nd_set_err(ND_ERR_ARG, "apgd control needs B, n_iter >= 1 and 1 <= C <= 1024 (C=%d)", C);
    if (iter < -1 || iter >= n_iter || k < 0 || k > iter + 1)
        return nd_set_err(ND_ERR_ARG, "apgd control needs -1 <= iter < n_iter and 0 <= k <= iter + 1 (iter=%d, k=%d, n_iter=%d)", iter, k, n_iter);
    hipLaunchKernelGGL(k_apgd_control, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, logits, labels, loss, step, loss_best,
                       loss_best_last_check, reduced_last_check, acc, loss_steps, flags, B, C, n_iter, iter, k, rho, step0);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_apgd_update(const float* x, float* x_adv, float* x_adv_old, const float* grad, float* x_best, float* grad_best, float* x_best_adv,
                              const int32_t* flags, const float* step, int B, size_t per_image, float eps, float a, int do_step, void* stream) {
    if (!x_adv || !grad) return nd_set_err(ND_ERR_ARG, "NULL tensor");
    if (flags && (!x_best || !grad_best || !x_best_adv)) return nd_set_err(ND_ERR_ARG, "apgd update with flags needs x_best, grad_best, x_best_adv");
    if (do_step && (!x || !x_adv_old || !step)) return nd_set_err(ND_ERR_ARG, "apgd update with a step needs x, x_adv_old, step");
    if (!flags && !do_step) return ND_OK;
    if (int rc = nd_check_rows("apgd update", B, per_image, 65535, LINF_MAX_QUADS)) return rc;
    const void* ptrs[] = {x, x_adv, x_adv_old, grad, x_best, grad_best, x_best_adv};
    for (const void* p : ptrs)
        if (nd_misaligned(p, 15)) return nd_set_err(ND_ERR_ARG, "apgd update needs 16-byte aligned images");
    const int quads = (int)(per_image / 4);
    const dim3 grid = nd_image_grid(B, quads, APGD_MAX_BLOCKS);
    hipStream_t st = (hipStream_t)stream;
    if (flags && do_step)
        hipLaunchKernelGGL((k_apgd_update<true, true>), grid, dim3(256), 0, st, x, x_adv, x_adv_old, grad, x_best, grad_best, x_best_adv, flags, step, quads, eps, a);
    else if (flags)
        hipLaunchKernelGGL((k_apgd_update<true, false>), grid, dim3(256), 0, st, x, x_adv, x_adv_old, grad, x_best, grad_best, x_best_adv, flags, step, quads, eps, a);
    else
        hipLaunchKernelGGL((k_apgd_update<false, true>), grid, dim3(256), 0, st, x, x_adv, x_adv_old, grad, x_best, grad_best, x_best_adv, flags, step, quads, eps, a);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}
