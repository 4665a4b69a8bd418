// nd_apgd_l2.hip -- AutoAttack's APGD with norm = 'L2' between two gradient passes (autopgd_base.py attack_single_run; the listing is in
// nested_diffusion_amd/autoattack.py), and the accumulation of an expectation over transformation (nested_diffusion_amd/eot.py).
// gfx950 only, all arithmetic fp32.  The per-image bookkeeping (nd_apgd_control) and the flags' copies (nd_apgd_update without a step)
// are norm-agnostic and stay in nd_attack_linf.hip.
//   k_apgd_l2_start_partial   per-workgroup partial of sum t^2 over the per_image Philox / Box-Muller normals of one image
//   k_apgd_l2_start           finishes tn = ||t||, out = clip(x0 + eps * (t / (tn + 1e-12)), lo, hi) (t recomputed)
//   k_apgd_l2_gsq             per-workgroup partial of sum g^2, g the row's gradient (grad_best in a restored row)
//   k_apgd_l2_d1              finishes gn, forms d1 = (xa + s * (g / (gn + 1e-12))) - x and its partial of sum d1^2
//   k_apgd_l2_d2              finishes n1, forms z, v and d2 = v - x (d1 recomputed) and its partial of sum d2^2
//   k_apgd_l2_apply           finishes n2, x_adv = clip(x + (d2 / (n2 + 1e-12)) * min(eps, n2), 0, 1), x_adv_old = xa (d2 recomputed)
//   k_eot_add                 acc = acc + g, or (acc + g) / divisor
//
// Row reductions have the fixed shape of nd_attack_l2.hip (nd_attack.hpp: grid (nd_l2_parts(per_image), B), one partial per workgroup,
// a finishing pass with the same xor tree, no floating-point atomics), so a norm has the same bits on every run and at every batch
// size.  The workspace holds two sets of partials: a pass reads the norms of the passes before the previous one from `norms`, where
// the previous pass wrote them, and so may overwrite their partials.
#include "nd_attack.hpp"
#include "nd_philox.hpp"

// every operation below is one rounded fp32 op in the listed order: a float32 restatement on the host reproduces the elementwise results
#pragma clang fp contract(off)

namespace {

constexpr int AL2_THREADS = ND_ATTACK_THREADS;
constexpr size_t AL2_MAX_QUADS = 0x7FFFFFFE;          // the limit of the L2 attack units

// ---- random start: Philox4x32-10 and Box-Muller (nd_philox.hpp), the word mapping of nd_l2_random_start ------------------------------
__device__ __forceinline__ float4 al2_draw(uint32_t image, uint32_t q, uint32_t restart, uint64_t seed) {
    uint32_t c[4] = {image, q, restart, ND_APGD_L2_START_TAG};
    nd_philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    float4 t;
    nd_box_muller(c[0], c[1], t.x, t.y);
    nd_box_muller(c[2], c[3], t.z, t.w);
    return t;
}

__global__ __launch_bounds__(AL2_THREADS) void k_apgd_l2_start_partial(const int64_t* __restrict__ index, float* __restrict__ part, int quads,
                                                                       uint64_t seed, uint32_t restart) {
    __shared__ float sh[4];
    const int b = blockIdx.y;
    const uint32_t image = (uint32_t)index[b];
    float s = 0.f;
    for (int q = blockIdx.x * AL2_THREADS + threadIdx.x; q < quads; q += gridDim.x * AL2_THREADS) s += l2_sq4(al2_draw(image, (uint32_t)q, restart, seed));
    s = l2_block_sum(s, sh);
    if (threadIdx.x == 0) part[(size_t)b * gridDim.x + blockIdx.x] = s;
}

__global__ __launch_bounds__(AL2_THREADS) void k_apgd_l2_start(const float* __restrict__ x0, const int64_t* __restrict__ index, float* __restrict__ out,
                                                               const float* __restrict__ part, float* __restrict__ tnorm, int quads, uint64_t seed,
                                                               uint32_t restart, float eps, float lo, float hi) {
    __shared__ float sh[4];
    const int b = blockIdx.y;
    const uint32_t image = (uint32_t)index[b];
    const float tn = sqrtf(l2_finish(part + (size_t)b * gridDim.x, gridDim.x, sh));
    if (blockIdx.x == 0 && threadIdx.x == 0) tnorm[b] = tn;
    const float den = tn + 1e-12f;
    const float4* a4 = reinterpret_cast<const float4*>(x0) + (size_t)b * quads;
    float4* o4 = reinterpret_cast<float4*>(out) + (size_t)b * quads;
    for (int q = blockIdx.x * AL2_THREADS + threadIdx.x; q < quads; q += gridDim.x * AL2_THREADS) {
        const float4 t = al2_draw(image, (uint32_t)q, restart, seed), a = a4[q];
        float4 r;
        r.x = nd_clampf(a.x + eps * (t.x / den), lo, hi);
        r.y = nd_clampf(a.y + eps * (t.y / den), lo, hi);
        r.z = nd_clampf(a.z + eps * (t.z / den), lo, hi);
        r.w = nd_clampf(a.w + eps * (t.w / den), lo, hi);
        o4[q] = r;
    }
}

// ---- the momentum step ---------------------------------------------------------------------------------------------------------------
// the per-image scalars of a row, workgroup-uniform
struct Al2Row {
    float s, gden, a, one_minus_a, eps;
    bool step;                                           // false: the gradient norm is NaN or infinite, u = xa
};

// the row's gradient: grad_best where the control kernel asked for a restore
__device__ __forceinline__ const float* al2_grad(const float* grad, const float* grad_best, const int32_t* flags, int b) {
    return (flags && (flags[b] & ND_APGD_RESTORE)) ? grad_best : grad;
}

__device__ __forceinline__ Al2Row al2_row(float gn, float s, float eps, float a) {
    Al2Row r;
    r.s = s; r.gden = gn + 1e-12f; r.a = a; r.one_minus_a = 1.0f - a; r.eps = eps;
    r.step = gn < INFINITY;
    return r;
}

// d1 = (xa + s * (g / (gn + 1e-12))) - x
__device__ __forceinline__ float al2_d1(float xa, float g, float x, const Al2Row& r) {
    const float u = r.step ? xa + r.s * (g / r.gden) : xa;
    return u - x;
}

// x + (d / (n + 1e-12)) * min(eps, n), clipped to [0, 1]: den = n + 1e-12, m = min(eps, n)
__device__ __forceinline__ float al2_project(float x, float d, float den, float m) { return nd_clampf(x + (d / den) * m, 0.f, 1.f); }

// d2 = ((xa + (z - xa) * a) + (xa - xold) * (1 - a)) - x, z the projection of d1
__device__ __forceinline__ float al2_d2(float xa, float xold, float g, float x, const Al2Row& r, float den1, float m1) {
    const float z = al2_project(x, al2_d1(xa, g, x, r), den1, m1);
    const float v = (xa + (z - xa) * r.a) + (xa - xold) * r.one_minus_a;
    return v - x;
}

__global__ __launch_bounds__(AL2_THREADS) void k_apgd_l2_gsq(const float* __restrict__ grad, const float* __restrict__ grad_best,
                                                             const int32_t* __restrict__ flags, float* __restrict__ part, int quads) {
    __shared__ float sh[4];
    const int b = blockIdx.y;
    const float4* g4 = reinterpret_cast<const float4*>(al2_grad(grad, grad_best, flags, b)) + (size_t)b * quads;
    float s = 0.f;
    for (int q = blockIdx.x * AL2_THREADS + threadIdx.x; q < quads; q += gridDim.x * AL2_THREADS) s += l2_sq4(g4[q]);
    s = l2_block_sum(s, sh);
    if (threadIdx.x == 0) part[(size_t)b * gridDim.x + blockIdx.x] = s;
}

__global__ __launch_bounds__(AL2_THREADS) void k_apgd_l2_d1(const float* __restrict__ x, const float* __restrict__ x_adv, const float* __restrict__ grad,
                                                            const float* __restrict__ grad_best, const int32_t* __restrict__ flags,
                                                            const float* __restrict__ step, const float* __restrict__ gpart, float* __restrict__ dpart,
                                                            float* __restrict__ norms, int quads, float eps, float a) {
    __shared__ float sh[4];
    const int b = blockIdx.y;
    const size_t base = (size_t)b * quads;
    const float gn = sqrtf(l2_finish(gpart + (size_t)b * gridDim.x, gridDim.x, sh));
    if (blockIdx.x == 0 && threadIdx.x == 0) norms[b] = gn;
    const Al2Row r = al2_row(gn, step[b], eps, a);
    const float4 *x4 = reinterpret_cast<const float4*>(x) + base, *xa4 = reinterpret_cast<const float4*>(x_adv) + base;
    const float4* g4 = reinterpret_cast<const float4*>(al2_grad(grad, grad_best, flags, b)) + base;
    float s = 0.f;
    for (int q = blockIdx.x * AL2_THREADS + threadIdx.x; q < quads; q += gridDim.x * AL2_THREADS) {
        const float4 xa = xa4[q], g = r.step ? g4[q] : float4{}, x0 = x4[q];
        float4 d;
        d.x = al2_d1(xa.x, g.x, x0.x, r); d.y = al2_d1(xa.y, g.y, x0.y, r); d.z = al2_d1(xa.z, g.z, x0.z, r); d.w = al2_d1(xa.w, g.w, x0.w, r);
        s += l2_sq4(d);
    }
    s = l2_block_sum(s, sh);
    if (threadIdx.x == 0) dpart[(size_t)b * gridDim.x + blockIdx.x] = s;
}

// gn comes from norms (written by k_apgd_l2_d1), so this pass may overwrite the gradient's partials with those of d2
__global__ __launch_bounds__(AL2_THREADS) void k_apgd_l2_d2(const float* __restrict__ x, const float* __restrict__ x_adv, const float* __restrict__ x_adv_old,
                                                            const float* __restrict__ grad, const float* __restrict__ grad_best,
                                                            const int32_t* __restrict__ flags, const float* __restrict__ step,
                                                            const float* __restrict__ d1part, float* __restrict__ d2part, float* __restrict__ norms,
                                                            int B, int quads, float eps, float a) {
    __shared__ float sh[4];
    const int b = blockIdx.y;
    const size_t base = (size_t)b * quads;
    const float n1 = sqrtf(l2_finish(d1part + (size_t)b * gridDim.x, gridDim.x, sh));
    if (blockIdx.x == 0 && threadIdx.x == 0) norms[(size_t)B + b] = n1;
    const Al2Row r = al2_row(norms[b], step[b], eps, a);
    const float den1 = n1 + 1e-12f, m1 = fminf(eps, n1);
    const float4 *x4 = reinterpret_cast<const float4*>(x) + base, *xa4 = reinterpret_cast<const float4*>(x_adv) + base;
    const float4* xo4 = reinterpret_cast<const float4*>(x_adv_old) + base;
    const float4* g4 = reinterpret_cast<const float4*>(al2_grad(grad, grad_best, flags, b)) + base;
    float s = 0.f;
    for (int q = blockIdx.x * AL2_THREADS + threadIdx.x; q < quads; q += gridDim.x * AL2_THREADS) {
        const float4 xa = xa4[q], xo = xo4[q], g = r.step ? g4[q] : float4{}, x0 = x4[q];
        float4 d;
        d.x = al2_d2(xa.x, xo.x, g.x, x0.x, r, den1, m1);
        d.y = al2_d2(xa.y, xo.y, g.y, x0.y, r, den1, m1);
        d.z = al2_d2(xa.z, xo.z, g.z, x0.z, r, den1, m1);
        d.w = al2_d2(xa.w, xo.w, g.w, x0.w, r, den1, m1);
        s += l2_sq4(d);
    }
    s = l2_block_sum(s, sh);
    if (threadIdx.x == 0) d2part[(size_t)b * gridDim.x + blockIdx.x] = s;
}

// x_adv and x_adv_old are read and written by the same thread, element by element (and may be one buffer on the first step)
__global__ __launch_bounds__(AL2_THREADS) void k_apgd_l2_apply(const float* __restrict__ x, float* x_adv, float* x_adv_old, const float* __restrict__ grad,
                                                               const float* __restrict__ grad_best, const int32_t* __restrict__ flags,
                                                               const float* __restrict__ step, const float* __restrict__ d2part, float* norms, int B,
                                                               int quads, float eps, float a) {
    __shared__ float sh[4];
    const int b = blockIdx.y;
    const size_t base = (size_t)b * quads;
    const float n2 = sqrtf(l2_finish(d2part + (size_t)b * gridDim.x, gridDim.x, sh));
    if (blockIdx.x == 0 && threadIdx.x == 0) norms[2 * (size_t)B + b] = n2;
    const Al2Row r = al2_row(norms[b], step[b], eps, a);
    const float n1 = norms[(size_t)B + b];
    const float den1 = n1 + 1e-12f, m1 = fminf(eps, n1), den2 = n2 + 1e-12f, m2 = fminf(eps, n2);
    const float4* x4 = reinterpret_cast<const float4*>(x) + base;
    float4 *xa4 = reinterpret_cast<float4*>(x_adv) + base, *xo4 = reinterpret_cast<float4*>(x_adv_old) + base;
    const float4* g4 = reinterpret_cast<const float4*>(al2_grad(grad, grad_best, flags, b)) + base;
    for (int q = blockIdx.x * AL2_THREADS + threadIdx.x; q < quads; q += gridDim.x * AL2_THREADS) {
        const float4 xa = xa4[q], xo = xo4[q], g = r.step ? g4[q] : float4{}, x0 = x4[q];
        float4 o;
        o.x = al2_project(x0.x, al2_d2(xa.x, xo.x, g.x, x0.x, r, den1, m1), den2, m2);
        o.y = al2_project(x0.y, al2_d2(xa.y, xo.y, g.y, x0.y, r, den1, m1), den2, m2);
        o.z = al2_project(x0.z, al2_d2(xa.z, xo.z, g.z, x0.z, r, den1, m1), den2, m2);
        o.w = al2_project(x0.w, al2_d2(xa.w, xo.w, g.w, x0.w, r, den1, m1), den2, m2);
        xo4[q] = xa;
        xa4[q] = o;
    }
}

// ---- expectation over transformation ---------------------------------------------------------------------------------------------------
template <bool DIVIDE>
__global__ __launch_bounds__(AL2_THREADS) void k_eot_add(float* __restrict__ acc, const float* __restrict__ g, size_t n4, float divisor) {
    for (size_t i = (size_t)blockIdx.x * AL2_THREADS + threadIdx.x; i < n4; i += (size_t)gridDim.x * AL2_THREADS) {
        const float4 a = reinterpret_cast<const float4*>(acc)[i], v = reinterpret_cast<const float4*>(g)[i];
        float4 r;
        r.x = a.x + v.x; r.y = a.y + v.y; r.z = a.z + v.z; r.w = a.w + v.w;
        if (DIVIDE) { r.x = r.x / divisor; r.y = r.y / divisor; r.z = r.z / divisor; r.w = r.w / divisor; }
        reinterpret_cast<float4*>(acc)[i] = r;
    }
}

}  // namespace

extern "C" int nd_apgd_l2_random_start(const float* x0, const int64_t* index, float* out, float* tnorm, float* ws, int B, size_t per_image,
                                       uint64_t seed, uint32_t restart, float eps, float lo, float hi, void* stream) {
    if (!x0 || !index || !out || !tnorm || !ws) return nd_set_err(ND_ERR_ARG, "nd_apgd_l2_random_start: NULL tensor");
    if (int rc = nd_check_rows("nd_apgd_l2_random_start", B, per_image, 65535, AL2_MAX_QUADS)) return rc;
    if (nd_misaligned(x0, 15) || nd_misaligned(out, 15)) return nd_set_err(ND_ERR_ARG, "nd_apgd_l2_random_start needs 16-byte aligned images");
    const int quads = (int)(per_image / 4);
    const dim3 grid = nd_image_grid(B, quads, ND_L2_MAX_PARTS), block(AL2_THREADS);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_apgd_l2_start_partial, grid, block, 0, st, index, ws, quads, seed, restart);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_apgd_l2_start, grid, block, 0, st, x0, index, out, ws, tnorm, quads, seed, restart, eps, lo, hi);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_apgd_l2_step(const float* x, float* x_adv, float* x_adv_old, const float* grad, const float* grad_best, const int32_t* flags,
                               const float* step, float* norms, float* ws, int B, size_t per_image, float eps, float a, void* stream) {
    if (!x || !x_adv || !x_adv_old || !grad || !step || !norms || !ws) return nd_set_err(ND_ERR_ARG, "nd_apgd_l2_step: NULL tensor");
    if (flags && !grad_best) return nd_set_err(ND_ERR_ARG, "nd_apgd_l2_step with flags needs grad_best");
    if (int rc = nd_check_rows("nd_apgd_l2_step", B, per_image, 65535, AL2_MAX_QUADS)) return rc;
    const void* ptrs[] = {x, x_adv, x_adv_old, grad, grad_best};
    for (const void* p : ptrs)
        if (nd_misaligned(p, 15)) return nd_set_err(ND_ERR_ARG, "nd_apgd_l2_step needs 16-byte aligned images");
    const int quads = (int)(per_image / 4);
    const dim3 grid = nd_image_grid(B, quads, ND_L2_MAX_PARTS), block(AL2_THREADS);
    float *p0 = ws, *p1 = ws + (size_t)B * ND_L2_MAX_PARTS;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_apgd_l2_gsq, grid, block, 0, st, grad, grad_best, flags, p0, quads);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_apgd_l2_d1, grid, block, 0, st, x, x_adv, grad, grad_best, flags, step, p0, p1, norms, quads, eps, a);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_apgd_l2_d2, grid, block, 0, st, x, x_adv, x_adv_old, grad, grad_best, flags, step, p1, p0, norms, B, quads, eps, a);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_apgd_l2_apply, grid, block, 0, st, x, x_adv, x_adv_old, grad, grad_best, flags, step, p0, norms, B, quads, eps, a);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_eot_add(float* acc, const float* g, size_t n, int divisor, void* stream) {
    if (!acc || !g) return nd_set_err(ND_ERR_ARG, "nd_eot_add: NULL tensor");
    if ((n % 4) || divisor < 0) return nd_set_err(ND_ERR_ARG, "nd_eot_add needs n %% 4 == 0 and divisor >= 0 (n=%zu, divisor=%d)", n, divisor);
    if (nd_misaligned(acc, 15) || nd_misaligned(g, 15)) return nd_set_err(ND_ERR_ARG, "nd_eot_add needs 16-byte aligned tensors");
    if (n == 0) return ND_OK;
    const size_t n4 = n / 4;
    const dim3 grid(nd_blocks_per_image(n4, 8192)), block(AL2_THREADS);
    if (divisor > 0)
        hipLaunchKernelGGL((k_eot_add<true>), grid, block, 0, (hipStream_t)stream, acc, g, n4, (float)divisor);
    else
        hipLaunchKernelGGL((k_eot_add<false>), grid, block, 0, (hipStream_t)stream, acc, g, n4, 0.f);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}
