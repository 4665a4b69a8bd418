// nd_attack_l2.hip -- the per-element and per-image passes of the L2 attacks (foolbox 3.x L2BasicIterativeAttack /
// L2ProjectedGradientDescentAttack) and of Carlini & Wagner's L2 attack (L2CarliniWagnerAttack) between two ViT passes; the listings are
// in nested_diffusion_amd/attack.py.  gfx950 only, all arithmetic fp32.
//   k_l2_sq_partial      per-workgroup partial of sum g^2 over one image
//   k_l2_delta_partial   finishes ||g||, forms d = (x + alpha * (g / ||g||)) - x0 and its per-workgroup partial of sum d^2
//   k_l2_project         finishes both norms, out = clip(x0 + d * min(1, eps / ||d||), lo, hi) (d recomputed: the same bits)
//   k_l2_start_partial   per-workgroup partial of sum z^2 over the n + 2 Philox / Box-Muller normals of one image
//   k_l2_start           finishes ||z||, out = clip(x0 + eps * (z / ||z||), lo, hi) (z recomputed)
//   k_cw_attack_space    w0 = atanh(((x0 - a) / b) * 0.999999), xrec = tanh(w0) * b + a
//   k_cw_model_space     t = tanh(w0 + delta), x = t * b + a, per-workgroup partials of sum (x - xrec)^2 and sum (x - x0)^2
//   k_l2_finish2         the finishing pass of those two sums
//   k_cw_control         per-image bookkeeping of one CW iteration (one thread per image)
//   k_cw_update          best-so-far copy, then the gradient in tanh space and the Adam update
//
// Row reductions have one fixed shape and no floating-point atomics: grid (nd_l2_parts(per_image), B); a thread sums its quads in grid-stride
// order, a workgroup folds its 256 threads by an xor-shuffle tree per wave and (w0 + w1) + (w2 + w3) over the waves, and writes one
// partial; the finishing pass folds the <= 256 partials of an image with the same tree.  The shape depends on per_image alone, so a sum
// has the same bits on every run, at every batch size and in every workgroup that finishes it.
#include "nd_attack.hpp"
#include "nd_philox.hpp"

// every operation below is one rounded fp32 op in the listed order: a float32 restatement on the host reproduces the elementwise results
#pragma clang fp contract(off)

namespace {

constexpr int L2_THREADS = ND_ATTACK_THREADS;

__global__ __launch_bounds__(L2_THREADS) void k_l2_sq_partial(const float* __restrict__ g, float* __restrict__ part, int quads) {
    __shared__ float sh[4];
    const int b = blockIdx.y;
    const float4* g4 = reinterpret_cast<const float4*>(g) + (size_t)b * quads;
    float s = 0.f;
    for (int q = blockIdx.x * L2_THREADS + threadIdx.x; q < quads; q += gridDim.x * L2_THREADS) s += l2_sq4(g4[q]);
    s = l2_block_sum(s, sh);
    if (threadIdx.x == 0) part[(size_t)b * gridDim.x + blockIdx.x] = s;
}

// d = (x + alpha * (g * inv)) - x0, or x - x0 without a step
__device__ __forceinline__ float4 l2_delta(float4 x, float4 g, float4 x0, bool step, float alpha, float inv) {
    float4 d;
    if (step) {
        d.x = (x.x + alpha * (g.x * inv)) - x0.x;
        d.y = (x.y + alpha * (g.y * inv)) - x0.y;
        d.z = (x.z + alpha * (g.z * inv)) - x0.z;
        d.w = (x.w + alpha * (g.w * inv)) - x0.w;
    } else {
        d.x = x.x - x0.x; d.y = x.y - x0.y; d.z = x.z - x0.z; d.w = x.w - x0.w;
    }
    return d;
}

// a row whose gradient norm is NaN (a NaN element) or infinite takes no step
__device__ __forceinline__ bool l2_takes_step(float gn) { return gn < INFINITY; }

__global__ __launch_bounds__(L2_THREADS) void k_l2_delta_partial(const float* __restrict__ x, const float* __restrict__ x0, const float* __restrict__ g,
                                                                 const float* __restrict__ gpart, float* __restrict__ dpart, float* __restrict__ gnorm,
                                                                 int quads, float alpha) {
    __shared__ float sh[4];
    const int b = blockIdx.y;
    const size_t base = (size_t)b * quads;
    float gn = 0.f;
    if (g) {
        gn = sqrtf(l2_finish(gpart + (size_t)b * gridDim.x, gridDim.x, sh));
        if (blockIdx.x == 0 && threadIdx.x == 0) gnorm[b] = gn;
    } else if (blockIdx.x == 0 && threadIdx.x == 0 && gnorm) gnorm[b] = 0.f;
    const bool step = g && l2_takes_step(gn);
    const float inv = 1.0f / fmaxf(gn, 1e-12f);
    const float4 *x4 = reinterpret_cast<const float4*>(x) + base, *a4 = reinterpret_cast<const float4*>(x0) + base;
    const float4* g4 = reinterpret_cast<const float4*>(g) + base;
    float s = 0.f;
    for (int q = blockIdx.x * L2_THREADS + threadIdx.x; q < quads; q += gridDim.x * L2_THREADS)
        s += l2_sq4(l2_delta(x4[q], step ? g4[q] : float4{}, a4[q], step, alpha, inv));
    s = l2_block_sum(s, sh);
    if (threadIdx.x == 0) dpart[(size_t)b * gridDim.x + blockIdx.x] = s;
}

__global__ __launch_bounds__(L2_THREADS) void k_l2_project(const float* __restrict__ x, const float* __restrict__ x0, const float* __restrict__ g,
                                                           float* __restrict__ out, const float* __restrict__ gpart, const float* __restrict__ dpart,
                                                           float* __restrict__ dnorm, int quads, float alpha, float eps, float lo, float hi) {
    __shared__ float sh[4];
    const int b = blockIdx.y;
    const size_t base = (size_t)b * quads;
    const float gn = g ? sqrtf(l2_finish(gpart + (size_t)b * gridDim.x, gridDim.x, sh)) : 0.f;
    const float dn = sqrtf(l2_finish(dpart + (size_t)b * gridDim.x, gridDim.x, sh));
    if (blockIdx.x == 0 && threadIdx.x == 0) dnorm[b] = dn;
    const bool step = g && l2_takes_step(gn);
    const float inv = 1.0f / fmaxf(gn, 1e-12f);
    const float f = fminf(1.0f, eps / fmaxf(dn, 1e-12f));
    const float4 *x4 = reinterpret_cast<const float4*>(x) + base, *a4 = reinterpret_cast<const float4*>(x0) + base;
    const float4* g4 = reinterpret_cast<const float4*>(g) + base;
    float4* o4 = reinterpret_cast<float4*>(out) + base;
    for (int q = blockIdx.x * L2_THREADS + threadIdx.x; q < quads; q += gridDim.x * L2_THREADS) {
        const float4 a = a4[q];
        const float4 d = l2_delta(x4[q], step ? g4[q] : float4{}, a, step, alpha, inv);
        float4 r;
        r.x = nd_clampf(a.x + d.x * f, lo, hi);
        r.y = nd_clampf(a.y + d.y * f, lo, hi);
        r.z = nd_clampf(a.z + d.z * f, lo, hi);
        r.w = nd_clampf(a.w + d.w * f, lo, hi);
        o4[q] = r;
    }
}

// ---- random start: Philox4x32-10 and Box-Muller (nd_philox.hpp) --------------------------------------------------------------------------
__device__ __forceinline__ float4 l2_draw(uint32_t image, uint32_t q, uint32_t restart, uint64_t seed) {
    uint32_t c[4] = {image, q, restart, ND_L2_START_TAG};
    nd_philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    float4 z;
    nd_box_muller(c[0], c[1], z.x, z.y);
    nd_box_muller(c[2], c[3], z.z, z.w);
    return z;
}

// quads 0 .. quads inclusive: the last one supplies normals n and n + 1 only
__global__ __launch_bounds__(L2_THREADS) void k_l2_start_partial(float* __restrict__ part, int quads, uint64_t seed, uint32_t first_image,
                                                                 uint32_t restart) {
    __shared__ float sh[4];
    const int b = blockIdx.y;
    const uint32_t image = first_image + (uint32_t)b;
    float s = 0.f;
    for (int q = blockIdx.x * L2_THREADS + threadIdx.x; q <= quads; q += gridDim.x * L2_THREADS) {
        float4 z = l2_draw(image, (uint32_t)q, restart, seed);
        if (q == quads) z.z = z.w = 0.f;
        s += l2_sq4(z);
    }
    s = l2_block_sum(s, sh);
    if (threadIdx.x == 0) part[(size_t)b * gridDim.x + blockIdx.x] = s;
}

__global__ __launch_bounds__(L2_THREADS) void k_l2_start(const float* __restrict__ x0, float* __restrict__ out, const float* __restrict__ part,
                                                         float* __restrict__ snorm, int quads, uint64_t seed, uint32_t first_image, uint32_t restart,
                                                         float eps, float lo, float hi) {
    __shared__ float sh[4];
    const int b = blockIdx.y;
    const uint32_t image = first_image + (uint32_t)b;
    const float sn = sqrtf(l2_finish(part + (size_t)b * gridDim.x, gridDim.x, sh));
    if (blockIdx.x == 0 && threadIdx.x == 0) snorm[b] = sn;
    const float4* a4 = reinterpret_cast<const float4*>(x0) + (size_t)b * quads;
    float4* o4 = reinterpret_cast<float4*>(out) + (size_t)b * quads;
    for (int q = blockIdx.x * L2_THREADS + threadIdx.x; q < quads; q += gridDim.x * L2_THREADS) {
        const float4 z = l2_draw(image, (uint32_t)q, restart, seed), a = a4[q];
        float4 r;
        r.x = nd_clampf(a.x + eps * (z.x / sn), lo, hi);
        r.y = nd_clampf(a.y + eps * (z.y / sn), lo, hi);
        r.z = nd_clampf(a.z + eps * (z.z / sn), lo, hi);
        r.w = nd_clampf(a.w + eps * (z.w / sn), lo, hi);
        o4[q] = r;
    }
}

// ---- Carlini & Wagner -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float cw_w0(float v, float a, float b) { return atanhf(((v - a) / b) * 0.999999f); }

__global__ __launch_bounds__(L2_THREADS) void k_cw_attack_space(const float* __restrict__ x0, float* __restrict__ w0, float* __restrict__ xrec,
                                                                size_t n4, float a, float b) {
    for (size_t i = (size_t)blockIdx.x * L2_THREADS + threadIdx.x; i < n4; i += (size_t)gridDim.x * L2_THREADS) {
        const float4 v = reinterpret_cast<const float4*>(x0)[i];
        float4 w, r;
        w.x = cw_w0(v.x, a, b); w.y = cw_w0(v.y, a, b); w.z = cw_w0(v.z, a, b); w.w = cw_w0(v.w, a, b);
        r.x = tanhf(w.x) * b + a; r.y = tanhf(w.y) * b + a; r.z = tanhf(w.z) * b + a; r.w = tanhf(w.w) * b + a;
        reinterpret_cast<float4*>(w0)[i] = w;
        reinterpret_cast<float4*>(xrec)[i] = r;
    }
}

__device__ __forceinline__ float4 sub4(float4 p, float4 q) { return make_float4(p.x - q.x, p.y - q.y, p.z - q.z, p.w - q.w); }

__global__ __launch_bounds__(L2_THREADS) void k_cw_model_space(const float* __restrict__ w0, const float* __restrict__ delta, const float* __restrict__ x0,
                                                               const float* __restrict__ xrec, float* __restrict__ t_out, float* __restrict__ x_out,
                                                               float* __restrict__ part_rec, float* __restrict__ part_x0, int quads, float a, float bh) {
    __shared__ float sh[4];
    const int b = blockIdx.y;
    const size_t base = (size_t)b * quads;
    float s_rec = 0.f, s_x0 = 0.f;
    for (int q = blockIdx.x * L2_THREADS + threadIdx.x; q < quads; q += gridDim.x * L2_THREADS) {
        const float4 w = reinterpret_cast<const float4*>(w0)[base + q], d = reinterpret_cast<const float4*>(delta)[base + q];
        float4 t, x;
        t.x = tanhf(w.x + d.x); t.y = tanhf(w.y + d.y); t.z = tanhf(w.z + d.z); t.w = tanhf(w.w + d.w);
        x.x = t.x * bh + a; x.y = t.y * bh + a; x.z = t.z * bh + a; x.w = t.w * bh + a;
        reinterpret_cast<float4*>(t_out)[base + q] = t;
        reinterpret_cast<float4*>(x_out)[base + q] = x;
        s_rec += l2_sq4(sub4(x, reinterpret_cast<const float4*>(xrec)[base + q]));
        s_x0 += l2_sq4(sub4(x, reinterpret_cast<const float4*>(x0)[base + q]));
    }
    s_rec = l2_block_sum(s_rec, sh);
    s_x0 = l2_block_sum(s_x0, sh);
    if (threadIdx.x == 0) {
        part_rec[(size_t)b * gridDim.x + blockIdx.x] = s_rec;
        part_x0[(size_t)b * gridDim.x + blockIdx.x] = s_x0;
    }
}

// one workgroup per image
__global__ __launch_bounds__(L2_THREADS) void k_l2_finish2(const float* __restrict__ part0, const float* __restrict__ part1, float* __restrict__ out0,
                                                           float* __restrict__ out1, int parts) {
    __shared__ float sh[4];
    const int b = blockIdx.x;
    const float s0 = l2_finish(part0 + (size_t)b * parts, parts, sh), s1 = l2_finish(part1 + (size_t)b * parts, parts, sh);
    if (threadIdx.x == 0) { out0[b] = s0; out1[b] = s1; }
}

__global__ __launch_bounds__(64) void k_cw_control(const float* __restrict__ logits, const int64_t* __restrict__ labels, const float* __restrict__ consts,
                                                   const float* __restrict__ margin, const float* __restrict__ sq_rec, const float* __restrict__ sq_x0,
                                                   float* __restrict__ best_norm, int32_t* __restrict__ found, int32_t* __restrict__ flags,
                                                   float* __restrict__ loss, int B, int C, float confidence) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float* l = logits + (size_t)b * C;
    const int64_t y = labels[b];
    int arg = 0;                                        // argmax(logits + confidence * onehot(label)): the first maximal index; a NaN never wins
    float best = 0 == y ? l[0] + confidence : l[0];
    for (int c = 1; c < C; ++c) {
        const float v = c == y ? l[c] + confidence : l[c];
        if (v > best || (best != best && v == v)) { best = v; arg = c; }
    }
    const bool adv = (int64_t)arg != y;
    const float norm = sqrtf(sq_x0[b]);
    const bool new_best = adv && norm < best_norm[b];
    if (adv) found[b] = 1;
    if (new_best) best_norm[b] = norm;
    flags[b] = new_best;
    const float m = margin[b];
    loss[b] = consts[b] * (m > 0.f ? m : 0.f) + sq_rec[b];
}

__device__ __forceinline__ void cw_adam(float& delta, float& m, float& v, float dx, float x, float xrec, float t, float stepsize, float bc1, float bc2,
                                        float bh) {
    const float g = ((dx + 2.0f * (x - xrec)) * bh) * (1.0f - t * t);
    m = 0.9f * m + 0.1f * g;
    v = 0.999f * v + 0.001f * (g * g);
    delta = delta - (stepsize * (m / bc1)) / (sqrtf(v / bc2) + 1e-8f);
}

__global__ __launch_bounds__(L2_THREADS) void k_cw_update(float* __restrict__ delta, float* __restrict__ m, float* __restrict__ v, const float* __restrict__ dx,
                                                          const float* __restrict__ x, const float* __restrict__ xrec, const float* __restrict__ t,
                                                          float* __restrict__ best, const int32_t* __restrict__ flags, int quads, float stepsize,
                                                          float bc1, float bc2, float bh) {
    const int b = blockIdx.y;
    const bool copy = flags && flags[b];
    const size_t base = (size_t)b * quads;
    for (int q = blockIdx.x * L2_THREADS + threadIdx.x; q < quads; q += gridDim.x * L2_THREADS) {
        const size_t i = base + q;
        const float4 xv = reinterpret_cast<const float4*>(x)[i], rv = reinterpret_cast<const float4*>(xrec)[i];
        const float4 tv = reinterpret_cast<const float4*>(t)[i], gv = reinterpret_cast<const float4*>(dx)[i];
        float4 d = reinterpret_cast<float4*>(delta)[i], mv = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
        if (copy) reinterpret_cast<float4*>(best)[i] = xv;
        cw_adam(d.x, mv.x, vv.x, gv.x, xv.x, rv.x, tv.x, stepsize, bc1, bc2, bh);
        cw_adam(d.y, mv.y, vv.y, gv.y, xv.y, rv.y, tv.y, stepsize, bc1, bc2, bh);
        cw_adam(d.z, mv.z, vv.z, gv.z, xv.z, rv.z, tv.z, stepsize, bc1, bc2, bh);
        cw_adam(d.w, mv.w, vv.w, gv.w, xv.w, rv.w, tv.w, stepsize, bc1, bc2, bh);
        reinterpret_cast<float4*>(delta)[i] = d;
        reinterpret_cast<float4*>(m)[i] = mv;
        reinterpret_cast<float4*>(v)[i] = vv;
    }
}

// the largest per_image / 4 the row check lets through: 0x7FFFFFFF itself is refused, because the start's loop runs to q <= quads
constexpr size_t L2_MAX_QUADS = 0x7FFFFFFE;

}  // namespace

// workgroups (and partials) per image: a function of per_image alone; enough of them to fill the chip at B = 1
extern "C" int nd_l2_parts(size_t per_image) {
    return (int)nd_blocks_per_image(per_image / 4, ND_L2_MAX_PARTS);
}

extern "C" int nd_l2_step(const float* x, const float* x0, const float* grad, float* out, float* gnorm, float* dnorm, float* ws, int B,
                          size_t per_image, float alpha, float eps, float lo, float hi, void* stream) {
    if (!x || !x0 || !out || !dnorm || !ws || (grad && !gnorm)) return nd_set_err(ND_ERR_ARG, "NULL tensor");
    if (int rc = nd_check_rows("l2 step", B, per_image, 65535, L2_MAX_QUADS)) return rc;
    if (nd_misaligned(x, 15) || nd_misaligned(x0, 15) || nd_misaligned(grad, 15) || nd_misaligned(out, 15))
        return nd_set_err(ND_ERR_ARG, "l2 step needs 16-byte aligned images");
    const int quads = (int)(per_image / 4);
    const dim3 grid = nd_image_grid(B, quads, ND_L2_MAX_PARTS), block(L2_THREADS);
    float *gpart = ws, *dpart = ws + (size_t)B * ND_L2_MAX_PARTS;
    hipStream_t st = (hipStream_t)stream;
    if (grad) {
        hipLaunchKernelGGL(k_l2_sq_partial, grid, block, 0, st, grad, gpart, quads);
        HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_l2_delta_partial, grid, block, 0, st, x, x0, grad, gpart, dpart, gnorm, quads, alpha);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_l2_project, grid, block, 0, st, x, x0, grad, out, gpart, dpart, dnorm, quads, alpha, eps, lo, hi);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_l2_random_start(const float* x0, float* out, float* snorm, float* ws, int B, size_t per_image, uint64_t seed, uint32_t first_image,
                                  uint32_t restart, float eps, float lo, float hi, void* stream) {
    if (!x0 || !out || !snorm || !ws) return nd_set_err(ND_ERR_ARG, "NULL tensor");
    if (int rc = nd_check_rows("l2 random start", B, per_image, 65535, L2_MAX_QUADS)) return rc;
    if (nd_misaligned(x0, 15) || nd_misaligned(out, 15)) return nd_set_err(ND_ERR_ARG, "l2 random start needs 16-byte aligned images");
    const int quads = (int)(per_image / 4);
    const dim3 grid = nd_image_grid(B, quads, ND_L2_MAX_PARTS), block(L2_THREADS);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_l2_start_partial, grid, block, 0, st, ws, quads, seed, first_image, restart);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_l2_start, grid, block, 0, st, x0, out, ws, snorm, quads, seed, first_image, restart, eps, lo, hi);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_cw_attack_space(const float* x0, float* w0, float* xrec, size_t n, float lo, float hi, void* stream) {
    if (!x0 || !w0 || !xrec) return nd_set_err(ND_ERR_ARG, "NULL tensor");
    if (n == 0 || (n % 4)) return nd_set_err(ND_ERR_ARG, "cw attack space needs n %% 4 == 0, n >= 4 (n=%zu)", n);
    if (!(hi > lo)) return nd_set_err(ND_ERR_ARG, "cw attack space needs bounds lo < hi");
    if (nd_misaligned(x0, 15) || nd_misaligned(w0, 15) || nd_misaligned(xrec, 15)) return nd_set_err(ND_ERR_ARG, "cw attack space needs 16-byte aligned tensors");
    const size_t n4 = n / 4;
    hipLaunchKernelGGL(k_cw_attack_space, dim3(nd_blocks_per_image(n4, 8192)), dim3(L2_THREADS), 0, (hipStream_t)stream, x0, w0, xrec, n4,
                       (lo + hi) / 2.0f, (hi - lo) / 2.0f);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_cw_model_space(const float* w0, const float* delta, const float* x0, const float* xrec, float* t_out, float* x_out, float* sq_rec,
                                 float* sq_x0, float* ws, int B, size_t per_image, float lo, float hi, void* stream) {
    if (!w0 || !delta || !x0 || !xrec || !t_out || !x_out || !sq_rec || !sq_x0 || !ws) return nd_set_err(ND_ERR_ARG, "NULL tensor");
    if (int rc = nd_check_rows("cw model space", B, per_image, 65535, L2_MAX_QUADS)) return rc;
    if (!(hi > lo)) return nd_set_err(ND_ERR_ARG, "cw model space needs bounds lo < hi");
    const void* ptrs[] = {w0, delta, x0, xrec, t_out, x_out};
    for (const void* p : ptrs)
        if (nd_misaligned(p, 15)) return nd_set_err(ND_ERR_ARG, "cw model space needs 16-byte aligned images");
    const int quads = (int)(per_image / 4);
    const dim3 grid = nd_image_grid(B, quads, ND_L2_MAX_PARTS);
    float *p_rec = ws, *p_x0 = ws + (size_t)B * ND_L2_MAX_PARTS;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_cw_model_space, grid, dim3(L2_THREADS), 0, st, w0, delta, x0, xrec, t_out, x_out, p_rec, p_x0,
                       quads, (lo + hi) / 2.0f, (hi - lo) / 2.0f);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_l2_finish2, dim3((unsigned)B), dim3(L2_THREADS), 0, st, p_rec, p_x0, sq_rec, sq_x0, (int)grid.x);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_cw_control(const float* logits, const int64_t* labels, const float* consts, const float* margin, const float* sq_rec,
                             const float* sq_x0, float* best_norm, int32_t* found, int32_t* flags, float* loss, int B, int C, float confidence,
                             void* stream) {
    if (!logits || !labels || !consts || !margin || !sq_rec || !sq_x0 || !best_norm || !found || !flags || !loss)
        return nd_set_err(ND_ERR_ARG, "NULL tensor");
    if (B < 1 || B > 65535 || C < 2 || C > 1024) return nd_set_err(ND_ERR_ARG, "cw control needs 1 <= B <= 65535 and 2 <= C <= 1024 (B=%d, C=%d)", B, C);
    hipLaunchKernelGGL(k_cw_control, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, logits, labels, consts, margin, sq_rec, sq_x0,
                       best_norm, found, flags, loss, B, C, confidence);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_cw_update(float* delta, float* m, float* v, const float* dx, const float* x, const float* xrec, const float* t, float* best,
                            const int32_t* flags, int B, size_t per_image, float stepsize, float bc1, float bc2, float b_half, void* stream) {
    if (!delta || !m || !v || !dx || !x || !xrec || !t || (flags && !best)) return nd_set_err(ND_ERR_ARG, "NULL tensor");
    if (int rc = nd_check_rows("cw update", B, per_image, 65535, L2_MAX_QUADS)) return rc;
    const void* ptrs[] = {delta, m, v, dx, x, xrec, t, best};
    for (const void* p : ptrs)
        if (nd_misaligned(p, 15)) return nd_set_err(ND_ERR_ARG, "cw update needs 16-byte aligned images");
    const int quads = (int)(per_image / 4);
    hipLaunchKernelGGL(k_cw_update, nd_image_grid(B, quads, ND_L2_MAX_PARTS), dim3(L2_THREADS), 0, (hipStream_t)stream, delta, m, v, dx, x,
                       xrec, t, best, flags, quads, stepsize, bc1, bc2, b_half);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}
