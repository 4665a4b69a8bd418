// nd_vit_grad.hip -- the input gradient of the full ViT (timm 0.4.12 VisionTransformer.forward, cross-entropy on the head) and the
// Linf attack steps built on it: what foolbox's LinfBaseGradientDescent asks of the model the reference attacks (attack.py;
// classification_train_separately.py:661-667, utils.py:258-269).  gfx950 only, all arithmetic fp32.
//
// Only the gradient with respect to the input image is formed; no weight gradient.  The Linear layers' input gradients
// dX = dY . W = dY . (W^T)^T are nd_gemm_split calls with the frag32b3 image of W^T as the weight operand (made once by the caller), so
// this file holds what is not a GEMM:
//   k_layernorm_bwd     LayerNorm input gradient (mean / rstd recomputed from the saved input), optional residual add; fp32 and/or image
//   k_gelu_split        GELU (the fc1 epilogue's expression) of the saved pre-activation, written as the fc2 operand image
//   k_gelu_bwd_split    du = dg * gelu'(u) (exact erf), written as the fc1-dX operand image
//   k_attention_bwd     dq, dk, dv of softmax(q k^T / 8) v for one (image, head) per workgroup: P recomputed from q and k
//   k_xent_head_bwd     softmax(logits) - onehot(label) times head.weight; per-image cross-entropy
//   k_margin_head_bwd   Carlini & Wagner's head: the gradient of c * max(0, logit margin) times head.weight; margin and runner-up
//   k_unpatchify        inverse permutation of k_patchify (stride == kernel: no overlap)
//   k_linf_step         x0 + clip(x + a sign(g) - x0, -eps, eps), clipped to the bounds (foolbox's order)
//   k_linf_start        x0 + U[-eps, eps) from Philox4x32-10, clipped to the bounds
//   k_apgd_start_max    AutoAttack APGD's random start, pass 1: per-image max |t| of the Philox draws (atomic max on the bit pattern)
//   k_apgd_start        pass 2: x0 + eps * t / (max|t| + 1e-12), the draws recomputed, clipped to the bounds
//   k_apgd_control      APGD's per-image bookkeeping of one iteration: acc, best loss, the checkpoint rule; writes the flags
//   k_apgd_update       APGD's per-element work of one iteration: best / best-adversarial copies, restore, the momentum step
#include "nd_common.hpp"
#include "nd_b9.hpp"
#include "nd_host.hpp"

// Every product below is rounded to fp32 before it is used: no contraction into a following add (in particular not into the first
// subtraction of nd_b9_split, which would make a frag32b3 image differ from the split of the fp32 value stored beside it).
#pragma clang fp contract(off)

// ---------------------------------------------------------------------------------------------
// LayerNorm backward, one wave per row: dx = rstd * (gg - mean(gg) - xh * mean(gg * xh)) (+ res), gg = g * gamma, xh = (x - mean) * rstd.
// The statistics are recomputed exactly as k_layernorm (nd_vit.hip) computes them (nd_ln_stats).
// ---------------------------------------------------------------------------------------------
template <int VPL>
__global__ __launch_bounds__(256) void k_layernorm_bwd(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ g,
                                                       const float* __restrict__ res, float* __restrict__ out, bf16x8* __restrict__ out_split,
                                                       int rows, int dim, float eps) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const size_t base = (size_t)row * dim;
    float4 v[VPL], gg[VPL];
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int c = (i * 64 + lane) * 4;
        v[i] = c < dim ? *reinterpret_cast<const float4*>(x + base + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float mean, cm, rstd;
    nd_ln_stats<VPL>(v, lane, dim, eps, mean, cm, rstd);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (c < dim) {
            const float4 gv = *reinterpret_cast<const float4*>(g + base + c);
            const float4 w = *reinterpret_cast<const float4*>(gamma + c);
            gg[i] = make_float4(gv.x * w.x, gv.y * w.y, gv.z * w.z, gv.w * w.w);
            v[i] = make_float4(((v[i].x - mean) - cm) * rstd, ((v[i].y - mean) - cm) * rstd, ((v[i].z - mean) - cm) * rstd, ((v[i].w - mean) - cm) * rstd);
            s1 += (gg[i].x + gg[i].y) + (gg[i].z + gg[i].w);
            s2 += (gg[i].x * v[i].x + gg[i].y * v[i].y) + (gg[i].z * v[i].z + gg[i].w * v[i].w);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s1 += __shfl_xor(s1, off, 64);
        s2 += __shfl_xor(s2, off, 64);
    }
    const float m1 = s1 / (float)dim, m2 = s2 / (float)dim;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (c < dim) {
            float4 o;
            o.x = rstd * (gg[i].x - m1 - v[i].x * m2);
            o.y = rstd * (gg[i].y - m1 - v[i].y * m2);
            o.z = rstd * (gg[i].z - m1 - v[i].z * m2);
            o.w = rstd * (gg[i].w - m1 - v[i].w * m2);
            if (res) {
                const float4 r = *reinterpret_cast<const float4*>(res + base + c);
                o.x += r.x; o.y += r.y; o.z += r.z; o.w += r.w;
            }
            if (out) *reinterpret_cast<float4*>(out + base + c) = o;
            if (out_split) nd_b9_store4(out_split, dim >> 5, row, c, o.x, o.y, o.z, o.w);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// GELU forward / backward written as frag32b3 images, one wave per (16 rows x 32 columns) block (the k_patchify_split pattern: a lane
// reads 8 consecutive values of its row, the wave writes three coalesced 1 KiB planes).  Rows past `rows` are written as zeros.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float nd_gelu_grad(float u) {
    // d/du [0.5 u (1 + erf(u / sqrt 2))] = 0.5 (1 + erf(u / sqrt 2)) + u exp(-u^2 / 2) / sqrt(2 pi)
    return 0.5f * (1.0f + nd_erf(u * 0.70710678118654752440f)) + u * 0.39894228040143267794f * expf(-0.5f * u * u);
}

template <bool BWD>
__global__ __launch_bounds__(256) void k_gelu_split(const float* __restrict__ u, const float* __restrict__ dg, float* __restrict__ out,
                                                    bf16x8* __restrict__ img, int rows, int cols) {
    const int lane = threadIdx.x & 63;
    const long blk = ((long)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int nkb = cols >> 5;
    if (blk >= (long)((rows + 15) >> 4) * nkb) return;
    const int rb = (int)(blk / nkb), kb = (int)(blk - (long)rb * nkb);
    const int r = rb * 16 + (lane & 15), c = kb * 32 + 8 * (lane >> 4);
    float v[8];
    if (r < rows) {
        const size_t o = (size_t)r * cols + c;
        const float4 u0 = *reinterpret_cast<const float4*>(u + o), u1 = *reinterpret_cast<const float4*>(u + o + 4);
        const float uu[8] = {u0.x, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w};
        if (BWD) {
            const float4 g0 = *reinterpret_cast<const float4*>(dg + o), g1 = *reinterpret_cast<const float4*>(dg + o + 4);
            const float gv[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = gv[e] * nd_gelu_grad(uu[e]);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = nd_act(uu[e], ND_ACT_GELU);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) asm("" : "+v"(v[e]));     // the rounded value: nd_act's last product must not fuse into the split
        if (out) {
            *reinterpret_cast<float4*>(out + o) = make_float4(v[0], v[1], v[2], v[3]);
            *reinterpret_cast<float4*>(out + o + 4) = make_float4(v[4], v[5], v[6], v[7]);
        }
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = 0.f;
    }
    bf16x8 h1, h2, h3;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        __bf16 a, b, cc;
        nd_b9_split(v[e], a, b, cc);
        h1[e] = a; h2[e] = b; h3[e] = cc;
    }
    img[(blk * 3 + 0) * 64 + lane] = h1;
    img[(blk * 3 + 1) * 64 + lane] = h2;
    img[(blk * 3 + 2) * 64 + lane] = h3;
}

// ---------------------------------------------------------------------------------------------
// Attention backward.  One workgroup (8 waves) per (image, head) holds all keys and values in LDS and sweeps the queries in slices of 16:
//   S = q k^T / 8, P = softmax(S) (recomputed: the forward keeps no statistics), dP = dO v^T, delta = rowsum(dO * O),
//   dS = P * (dP - delta);  dV += P^T dO,  dK += dS^T q / 8 (register accumulators across every slice),  dQ = dS k / 8 (per slice).
// dK and dV are complete when the sweep ends, so there are no atomics and the result is bitwise reproducible.  fp32 FMAs throughout.
// ---------------------------------------------------------------------------------------------
#define ATB_NMAX 208            // keys per (image, head): N <= 208 (197 for ViT-B/16 at 224^2)
#define ATB_QS 16               // query rows per slice
#define ATB_KS 68               // LDS row stride (floats) of K, V, q, dO: 17 16-byte units -> conflict-free ds_read_b128 down a column
#define ATB_PS 224              // LDS row stride of P / dS: >= 32 * 7, the keys the dK / dV accumulators cover
#define ATB_THREADS 512
#define ATB_LDS_FLOATS (2 * ATB_NMAX * ATB_KS + 2 * ATB_QS * ATB_KS + 2 * ATB_QS * ATB_PS + ATB_QS + 256 * 4)

__global__ __launch_bounds__(ATB_THREADS) void k_attention_bwd(const float* __restrict__ qkv, const float* __restrict__ o,
                                                               const float* __restrict__ dout, float* __restrict__ dqkv,
                                                               bf16x8* __restrict__ dqkv_split, int N, int heads) {
    extern __shared__ __attribute__((aligned(16))) float atb[];
    float* Ks = atb;                                  // [NMAX][KS]
    float* Vs = Ks + ATB_NMAX * ATB_KS;               // [NMAX][KS]
    float* Qs = Vs + ATB_NMAX * ATB_KS;               // [QS][KS]
    float* dOs = Qs + ATB_QS * ATB_KS;                // [QS][KS]
    float* Ps = dOs + ATB_QS * ATB_KS;                // [QS][PS]: scores, then probabilities
    float* dSs = Ps + ATB_QS * ATB_PS;               // [QS][PS]: dP, then dS
    float* delta = dSs + ATB_QS * ATB_PS;            // [QS]
    float* dQx = delta + ATB_QS;                      // [256][4]: upper half's partial dQ

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
    const int E = heads * 64, RS = 3 * E;
    const size_t row0 = (size_t)b * N;
    const int qoff = h * 64, koff = E + h * 64, voff = 2 * E + h * 64;

    for (int idx = t; idx < N * 16; idx += ATB_THREADS) {
        const int n = idx >> 4, c = (idx & 15) * 4;
        const float* src = qkv + (row0 + n) * RS;
        *reinterpret_cast<float4*>(Ks + n * ATB_KS + c) = *reinterpret_cast<const float4*>(src + koff + c);
        *reinterpret_cast<float4*>(Vs + n * ATB_KS + c) = *reinterpret_cast<const float4*>(src + voff + c);
    }

    const int c4 = t & 15, g = t >> 4;                // dK / dV ownership: columns 4*c4 .. +3 of keys g + 32 m
    float4 dK[7], dV[7];
#pragma unroll
    for (int m = 0; m < 7; ++m) dK[m] = dV[m] = make_float4(0.f, 0.f, 0.f, 0.f);
    const int nkb = RS >> 5;

    for (int s0 = 0; s0 < N; s0 += ATB_QS) {
        const int ns = min(ATB_QS, N - s0);
        __syncthreads();                              // previous slice done with Qs / dOs / Ps / dSs (and K, V staged on the first)
        if (t < ATB_QS * 16) {
            const int i = t >> 4, c = c4 * 4;
            float4 q4 = make_float4(0.f, 0.f, 0.f, 0.f), d4 = q4, o4 = q4;
            if (i < ns) {
                const size_t r = row0 + s0 + i;
                q4 = *reinterpret_cast<const float4*>(qkv + r * RS + qoff + c);
                d4 = *reinterpret_cast<const float4*>(dout + r * E + h * 64 + c);
                o4 = *reinterpret_cast<const float4*>(o + r * E + h * 64 + c);
            }
            *reinterpret_cast<float4*>(Qs + i * ATB_KS + c) = q4;
            *reinterpret_cast<float4*>(dOs + i * ATB_KS + c) = d4;
            float dd = (d4.x * o4.x + d4.y * o4.y) + (d4.z * o4.z + d4.w * o4.w);
#pragma unroll
            for (int off = 8; off > 0; off >>= 1) dd += __shfl_xor(dd, off, 64);
            if (c4 == 0) delta[i] = dd;
        }
        __syncthreads();
        // phase 1: S and dP; thread = key j, 8 query rows
        {
            const int j = t & 255, i0 = (t >> 8) * 8;
            if (j < N) {
                float sc[8], dp[8];
#pragma unroll
                for (int r = 0; r < 8; ++r) sc[r] = dp[r] = 0.f;
#pragma unroll 4
                for (int c = 0; c < 64; c += 4) {
                    const float4 k4 = *reinterpret_cast<const float4*>(Ks + j * ATB_KS + c);
                    const float4 v4 = *reinterpret_cast<const float4*>(Vs + j * ATB_KS + c);
#pragma unroll
                    for (int r = 0; r < 8; ++r) {
                        const float4 q4 = *reinterpret_cast<const float4*>(Qs + (i0 + r) * ATB_KS + c);
                        const float4 d4 = *reinterpret_cast<const float4*>(dOs + (i0 + r) * ATB_KS + c);
                        sc[r] = __builtin_fmaf(q4.x, k4.x, sc[r]); sc[r] = __builtin_fmaf(q4.y, k4.y, sc[r]);
                        sc[r] = __builtin_fmaf(q4.z, k4.z, sc[r]); sc[r] = __builtin_fmaf(q4.w, k4.w, sc[r]);
                        dp[r] = __builtin_fmaf(d4.x, v4.x, dp[r]); dp[r] = __builtin_fmaf(d4.y, v4.y, dp[r]);
                        dp[r] = __builtin_fmaf(d4.z, v4.z, dp[r]); dp[r] = __builtin_fmaf(d4.w, v4.w, dp[r]);
                    }
                }
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    Ps[(i0 + r) * ATB_PS + j] = sc[r] * 0.125f;
                    dSs[(i0 + r) * ATB_PS + j] = dp[r];
                }
            }
        }
        __syncthreads();
        // phase 2: softmax and dS, one wave per row (rows past ns become zeros: they add nothing below)
        for (int i = wave; i < ATB_QS; i += ATB_THREADS / 64) {
            float sv[4], mx = -INFINITY;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int j = lane + 64 * m;
                sv[m] = (i < ns && j < N) ? Ps[i * ATB_PS + j] : -INFINITY;
                mx = fmaxf(mx, sv[m]);
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
            float sum = 0.f;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                sv[m] = (i < ns && lane + 64 * m < N) ? expf(sv[m] - mx) : 0.f;
                sum += sv[m];
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
            const float inv = i < ns ? 1.0f / sum : 0.f, dl = delta[i];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int j = lane + 64 * m;
                if (j < ATB_PS) {
                    const float p = sv[m] * inv;
                    const float dsv = j < N && i < ns ? p * (dSs[i * ATB_PS + j] - dl) : 0.f;
                    Ps[i * ATB_PS + j] = p;
                    dSs[i * ATB_PS + j] = dsv;
                }
            }
        }
        __syncthreads();
        // phase 3a: dV += P^T dO, dK += dS^T q over this slice's rows
#pragma unroll 2
        for (int i = 0; i < ATB_QS; ++i) {
            const float4 d4 = *reinterpret_cast<const float4*>(dOs + i * ATB_KS + c4 * 4);
            const float4 q4 = *reinterpret_cast<const float4*>(Qs + i * ATB_KS + c4 * 4);
#pragma unroll
            for (int m = 0; m < 7; ++m) {
                const float p = Ps[i * ATB_PS + g + 32 * m], dsv = dSs[i * ATB_PS + g + 32 * m];
                dV[m].x = __builtin_fmaf(p, d4.x, dV[m].x); dV[m].y = __builtin_fmaf(p, d4.y, dV[m].y);
                dV[m].z = __builtin_fmaf(p, d4.z, dV[m].z); dV[m].w = __builtin_fmaf(p, d4.w, dV[m].w);
                dK[m].x = __builtin_fmaf(dsv, q4.x, dK[m].x); dK[m].y = __builtin_fmaf(dsv, q4.y, dK[m].y);
                dK[m].z = __builtin_fmaf(dsv, q4.z, dK[m].z); dK[m].w = __builtin_fmaf(dsv, q4.w, dK[m].w);
            }
        }
        // phase 3b: dQ = dS k / 8; the two thread halves take the lower / upper keys, the upper half's partial goes through LDS
        {
            const int half = t >> 8, i = (t & 255) >> 4;
            const int jm = (N + 1) >> 1, j0 = half ? jm : 0, j1 = half ? N : jm;
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int j = j0; j < j1; ++j) {
                const float dsv = dSs[i * ATB_PS + j];
                const float4 k4 = *reinterpret_cast<const float4*>(Ks + j * ATB_KS + c4 * 4);
                a.x = __builtin_fmaf(dsv, k4.x, a.x); a.y = __builtin_fmaf(dsv, k4.y, a.y);
                a.z = __builtin_fmaf(dsv, k4.z, a.z); a.w = __builtin_fmaf(dsv, k4.w, a.w);
            }
            if (half) *reinterpret_cast<float4*>(dQx + (t & 255) * 4) = a;
            __syncthreads();
            if (!half && i < ns) {
                const float4 u = *reinterpret_cast<const float4*>(dQx + t * 4);
                const float4 r = make_float4((a.x + u.x) * 0.125f, (a.y + u.y) * 0.125f, (a.z + u.z) * 0.125f, (a.w + u.w) * 0.125f);
                const size_t row = row0 + s0 + i;
                const int col = qoff + c4 * 4;
                if (dqkv) *reinterpret_cast<float4*>(dqkv + row * RS + col) = r;
                if (dqkv_split) nd_b9_store4(dqkv_split, nkb, (int)row, col, r.x, r.y, r.z, r.w);
            }
        }
    }
#pragma unroll
    for (int m = 0; m < 7; ++m) {
        const int j = g + 32 * m;
        if (j < N) {
            const size_t row = row0 + j;
            const float4 k = make_float4(dK[m].x * 0.125f, dK[m].y * 0.125f, dK[m].z * 0.125f, dK[m].w * 0.125f);
            if (dqkv) {
                *reinterpret_cast<float4*>(dqkv + row * RS + koff + c4 * 4) = k;
                *reinterpret_cast<float4*>(dqkv + row * RS + voff + c4 * 4) = dV[m];
            }
            if (dqkv_split) {
                nd_b9_store4(dqkv_split, nkb, (int)row, koff + c4 * 4, k.x, k.y, k.z, k.w);
                nd_b9_store4(dqkv_split, nkb, (int)row, voff + c4 * 4, dV[m].x, dV[m].y, dV[m].z, dV[m].w);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Cross-entropy and head: d = softmax(logits) - onehot(label) (foolbox: crossentropy(logits, labels).sum()), dfeat = d . head_w
// ([C, E] row-major), loss = logsumexp(logits) - logits[label].  One workgroup per image.
// d is formed in fp32 as p - 1 at the label: once 1 - p_y < 2^-24 it is 0 there, as in torch's fp32 softmax and the foolbox loop.
// The label's own term joins the sum last: summed in a lane, its e^0 = 1 of a confident head made every later term round at ulp(1).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_xent_head_bwd(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                       const float* __restrict__ w, float* __restrict__ dfeat, float* __restrict__ loss,
                                                       int C, int E) {
    __shared__ float d[1024];
    __shared__ float red[2];
    const int b = blockIdx.x, t = threadIdx.x;
    const float* l = logits + (size_t)b * C;
    const int64_t y = labels[b];
    if (t < 64) {
        float mx = -INFINITY;
        for (int c = t; c < C; c += 64) mx = fmaxf(mx, l[c]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
        float s = 0.f;
        for (int c = t; c < C; c += 64)
            if (c != y) s += expf(l[c] - mx);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        if (t == 0) { red[0] = mx; red[1] = (y >= 0 && y < C) ? s + expf(l[y] - mx) : s; }
    }
    __syncthreads();
    const float mx = red[0], inv = 1.0f / red[1];
    for (int c = t; c < C; c += 256) d[c] = expf(l[c] - mx) * inv - (c == y ? 1.0f : 0.0f);
    if (t == 0 && loss) loss[b] = (logf(red[1]) + mx) - ((y >= 0 && y < C) ? l[y] : NAN);
    __syncthreads();
    for (int e = t; e < E; e += 256) {
        float a = 0.f;
        for (int c = 0; c < C; ++c) a = __builtin_fmaf(d[c], w[(size_t)c * E + e], a);
        dfeat[(size_t)b * E + e] = a;
    }
}

// ---------------------------------------------------------------------------------------------
// Carlini & Wagner's head: the gradient of c * max(0, margin), margin = logits[label] - logits[other] + confidence, other = the first
// maximal index over the non-label columns (a NaN logit never wins; no number among them: the first non-label column).  dlogits is +c at
// the label and -c at other where margin > 0, else 0 (at margin == 0 the gradient is 0, where torch's maximum passes half);
// dfeat = dlogits . head_w, the two terms joined in column order as a sum over all columns would.  One workgroup per image; a label
// outside [0, C) gives margin NaN, other -1 and a zero gradient.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_margin_head_bwd(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                         const float* __restrict__ consts, const float* __restrict__ w, float* __restrict__ dfeat,
                                                         float* __restrict__ margin, int32_t* __restrict__ other, int C, int E, float confidence) {
    __shared__ int s_other;
    __shared__ float s_margin;
    const int b = blockIdx.x, t = threadIdx.x;
    const float* l = logits + (size_t)b * C;
    const int64_t y = labels[b];
    const bool valid = y >= 0 && y < C;
    if (t < 64) {
        int arg = 0x7FFFFFFF;                            // no number seen yet
        float best = 0.f;
        for (int c = t; c < C; c += 64) {
            const float v = l[c];
            if (c != y && v == v && (arg == 0x7FFFFFFF || v > best)) { best = v; arg = c; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(best, off, 64);
            const int oa = __shfl_xor(arg, off, 64);
            if (oa != 0x7FFFFFFF && (arg == 0x7FFFFFFF || ov > best || (ov == best && oa < arg))) { best = ov; arg = oa; }
        }
        if (t == 0) {
            if (arg == 0x7FFFFFFF) arg = y == 0 ? 1 : 0;
            s_other = valid ? arg : -1;
            s_margin = valid ? (l[y] - l[arg]) + confidence : NAN;
            other[b] = s_other;
            margin[b] = s_margin;
        }
    }
    __syncthreads();
    const float c = consts[b];
    const bool on = s_margin > 0.f;
    const int o = s_other, yi = (int)y;
    const int c1 = yi < o ? yi : o, c2 = yi < o ? o : yi;
    const float d1 = yi < o ? c : -c, d2 = yi < o ? -c : c;
    for (int e = t; e < E; e += 256) {
        float a = 0.f;
        if (on) {
            a = __builtin_fmaf(d1, w[(size_t)c1 * E + e], a);
            a = __builtin_fmaf(d2, w[(size_t)c2 * E + e], a);
        }
        dfeat[(size_t)b * E + e] = a;
    }
}

// ---------------------------------------------------------------------------------------------
// un-patchify: img[b][c][py*p+iy][px*p+ix] = cols[(b, py, px)][c*p*p + iy*p + ix]; 4 consecutive pixels of a row per thread
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_unpatchify(const float* __restrict__ cols, float* __restrict__ img, int B, int Cin, int Himg, int Wimg, int p) {
    const int gw = Wimg / p, gh = Himg / p;
    const size_t total4 = (size_t)B * Cin * Himg * Wimg / 4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (size_t)gridDim.x * blockDim.x) {
        const size_t e = i * 4;
        const int x = (int)(e % Wimg), y = (int)((e / Wimg) % Himg);
        const size_t bc = e / ((size_t)Wimg * Himg);
        const int c = (int)(bc % Cin), b = (int)(bc / Cin);
        const size_t tok = ((size_t)b * gh + y / p) * gw + x / p;
        const int col = (c * p + y % p) * p + x % p;
        *reinterpret_cast<float4*>(img + e) = *reinterpret_cast<const float4*>(cols + tok * ((size_t)Cin * p * p) + col);
    }
}

// ---------------------------------------------------------------------------------------------
// Linf steps.  Every operation is a single rounded fp32 op in foolbox's order (contraction is off in this file; the __f*_rn helpers of
// the HIP headers are not used: their multiply and add fuse into an FMA), so a float32 restatement on the host reproduces them bit for bit.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float nd_clampf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

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

__device__ __forceinline__ void nd_philox4x32_10_g(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// one thread per 4 elements of one image (per_image % 4 == 0); see nd_linf_random_start in the header for the mapping
__global__ __launch_bounds__(256) void k_linf_start(const float* __restrict__ x0, float* __restrict__ out, int B, int quads, uint64_t seed,
                                                    uint32_t first_image, uint32_t restart, float eps, float lo, float hi) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)B * quads) return;
    const int b = (int)(idx / quads), q = (int)(idx - (size_t)b * quads);
    uint32_t c[4] = {first_image + (uint32_t)b, (uint32_t)q, restart, ND_LINF_START_TAG};
    nd_philox4x32_10_g(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const size_t o = idx * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float u = (float)(c[e] >> 8) * 5.9604644775390625e-8f;                  // [0, 1), 24 bits: exact
        const float w = 2.0f * u - 1.0f;                                               // [-1, 1): exact
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
    nd_philox4x32_10_g(c, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
    for (int e = 0; e < 4; ++e) t[e] = 2.0f * ((float)(c[e] >> 8) * 5.9604644775390625e-8f) - 1.0f;   // 2u - 1: exact
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
static unsigned grid_for(size_t n) {
    const size_t b = (n + 255) / 256;
    return (unsigned)(b > 8192 ? 8192 : (b ? b : 1));
}

extern "C" int nd_layernorm_bwd(const float* x, const float* gamma, const float* g, const float* residual, float* out, void* out_split,
                                int rows, int dim, float eps, void* stream) {
    if (!x || !gamma || !g || (!out && !out_split)) return nd_set_err(ND_ERR_ARG, "NULL tensor");
    if (rows < 1 || dim < 4 || (dim % 4) || dim > 2048) return nd_set_err(ND_ERR_ARG, "layernorm_bwd needs dim %% 4 == 0, 4 <= dim <= 2048");
    if (out_split && (dim % 32)) return nd_set_err(ND_ERR_ARG, "a split (frag32b3) output needs dim %% 32 == 0");
    const int vpl = (dim + 255) / 256;
    const dim3 grid((rows + 3) / 4), block(256);
    hipStream_t st = (hipStream_t)stream;
    bf16x8* os = reinterpret_cast<bf16x8*>(out_split);
    if (vpl <= 1) hipLaunchKernelGGL((k_layernorm_bwd<1>), grid, block, 0, st, x, gamma, g, residual, out, os, rows, dim, eps);
    else if (vpl <= 2) hipLaunchKernelGGL((k_layernorm_bwd<2>), grid, block, 0, st, x, gamma, g, residual, out, os, rows, dim, eps);
    else if (vpl <= 3) hipLaunchKernelGGL((k_layernorm_bwd<3>), grid, block, 0, st, x, gamma, g, residual, out, os, rows, dim, eps);
    else if (vpl <= 4) hipLaunchKernelGGL((k_layernorm_bwd<4>), grid, block, 0, st, x, gamma, g, residual, out, os, rows, dim, eps);
    else hipLaunchKernelGGL((k_layernorm_bwd<8>), grid, block, 0, st, x, gamma, g, residual, out, os, rows, dim, eps);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

static int gelu_any(const float* u, const float* dg, float* out, void* out_split, int rows, int cols, bool bwd, void* stream) {
    if (!u || !out_split || (bwd && !dg)) return nd_set_err(ND_ERR_ARG, "NULL tensor");
    if (rows < 1 || cols < 32 || (cols % 32)) return nd_set_err(ND_ERR_ARG, "gelu images need cols %% 32 == 0 (cols=%d)", cols);
    const long nb = (long)((rows + 15) / 16) * (cols / 32);
    const dim3 grid((unsigned)((nb * 64 + 255) / 256));
    if (bwd) hipLaunchKernelGGL((k_gelu_split<true>), grid, dim3(256), 0, (hipStream_t)stream, u, dg, out, reinterpret_cast<bf16x8*>(out_split), rows, cols);
    else hipLaunchKernelGGL((k_gelu_split<false>), grid, dim3(256), 0, (hipStream_t)stream, u, dg, out, reinterpret_cast<bf16x8*>(out_split), rows, cols);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_gelu_split(const float* u, float* out, void* out_split, int rows, int cols, void* stream) {
    return gelu_any(u, nullptr, out, out_split, rows, cols, false, stream);
}

extern "C" int nd_gelu_bwd_split(const float* u, const float* dg, float* out, void* out_split, int rows, int cols, void* stream) {
    return gelu_any(u, dg, out, out_split, rows, cols, true, stream);
}

extern "C" int nd_attention_bwd(const float* qkv, const float* o, const float* dout, float* dqkv, void* dqkv_split, int B, int N, int heads,
                                void* stream) {
    if (!qkv || !o || !dout || (!dqkv && !dqkv_split)) return nd_set_err(ND_ERR_ARG, "NULL tensor");
    if (B < 1 || N < 1 || N > ATB_NMAX || heads < 1) return nd_set_err(ND_ERR_ARG, "attention_bwd needs 1 <= N <= %d, B, heads >= 1 (N=%d)", ATB_NMAX, N);
    const size_t lds = (size_t)ATB_LDS_FLOATS * sizeof(float);
    HIP_CHECK(nd_allow_dynamic_lds((const void*)k_attention_bwd, lds));
    hipLaunchKernelGGL(k_attention_bwd, dim3((unsigned)(B * heads)), dim3(ATB_THREADS), lds, (hipStream_t)stream, qkv, o, dout, dqkv,
                       reinterpret_cast<bf16x8*>(dqkv_split), N, heads);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_xent_head_bwd(const float* logits, const int64_t* labels, const float* head_w, float* dfeat, float* loss, int B, int C, int E,
                                void* stream) {
    if (!logits || !labels || !head_w || !dfeat) return nd_set_err(ND_ERR_ARG, "NULL tensor");
    if (B < 1 || C < 1 || C > 1024 || E < 1) return nd_set_err(ND_ERR_ARG, "xent_head_bwd needs 1 <= C <= 1024 (C=%d)", C);
    hipLaunchKernelGGL(k_xent_head_bwd, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, logits, labels, head_w, dfeat, loss, C, E);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_margin_head_bwd(const float* logits, const int64_t* labels, const float* consts, const float* head_w, float* dfeat,
                                  float* margin, int32_t* other, int B, int C, int E, float confidence, void* stream) {
    if (!logits || !labels || !consts || !head_w || !dfeat || !margin || !other) return nd_set_err(ND_ERR_ARG, "NULL tensor");
    if (B < 1 || C < 2 || C > 1024 || E < 1) return nd_set_err(ND_ERR_ARG, "margin_head_bwd needs 2 <= C <= 1024 (C=%d)", C);
    hipLaunchKernelGGL(k_margin_head_bwd, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, logits, labels, consts, head_w, dfeat, margin, other,
                       C, E, confidence);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_unpatchify(const float* cols, float* img, int B, int Cin, int Himg, int Wimg, int p, void* stream) {
    if (!cols || !img) return nd_set_err(ND_ERR_ARG, "NULL tensor");
    if (B < 1 || Cin < 1 || p < 4 || (p % 4) || Himg % p || Wimg % p) return nd_set_err(ND_ERR_ARG, "patch size must be a multiple of 4 dividing the image");
    const size_t total4 = (size_t)B * Cin * Himg * Wimg / 4;
    hipLaunchKernelGGL(k_unpatchify, dim3(grid_for(total4)), dim3(256), 0, (hipStream_t)stream, cols, img, B, Cin, Himg, Wimg, p);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_linf_step(const float* x, const float* x0, const float* grad, float* out, size_t n, float alpha, float eps, float lo, float hi,
                            void* stream) {
    if (!x || !x0 || !out) return nd_set_err(ND_ERR_ARG, "NULL tensor");
    if (n == 0) return ND_OK;
    hipLaunchKernelGGL(k_linf_step, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, x, x0, grad, out, n, alpha, eps, lo, hi);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_linf_random_start(const float* x0, float* out, int B, size_t per_image, uint64_t seed, uint32_t first_image, uint32_t restart,
                                    float eps, float lo, float hi, void* stream) {
    if (!x0 || !out) return nd_set_err(ND_ERR_ARG, "NULL tensor");
    if (B < 1 || per_image == 0 || (per_image % 4) || per_image / 4 > 0x7FFFFFFF)
        return nd_set_err(ND_ERR_ARG, "random start needs per_image %% 4 == 0");
    const int quads = (int)(per_image / 4);
    const size_t n = (size_t)B * quads;
    hipLaunchKernelGGL(k_linf_start, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x0, out, B, quads, seed, first_image, restart,
                       eps, lo, hi);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

static bool nd_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// (blocks per image, images): enough workgroups per image to fill the chip at B = 1, grid-stride beyond
static dim3 apgd_grid(int B, int quads) {
    const int per = (quads + 255) / 256;
    return dim3((unsigned)(per > 1024 ? 1024 : per), (unsigned)B);
}

extern "C" int nd_apgd_random_start(const float* x0, const int64_t* index, float* out, uint32_t* m_ws, int B, size_t per_image, uint64_t seed,
                                    uint32_t restart, float eps, float lo, float hi, void* stream) {
    if (!x0 || !index || !out || !m_ws) return nd_set_err(ND_ERR_ARG, "NULL tensor");
    if (B < 1 || B > 65535 || per_image == 0 || (per_image % 4) || per_image / 4 > 0x7FFFFFFF)
        return nd_set_err(ND_ERR_ARG, "apgd random start needs 1 <= B <= 65535 and per_image %% 4 == 0");
    if (!nd_aligned16(x0) || !nd_aligned16(out)) return nd_set_err(ND_ERR_ARG, "apgd random start needs 16-byte aligned images");
    const int quads = (int)(per_image / 4);
    hipStream_t st = (hipStream_t)stream;
    HIP_CHECK(hipMemsetAsync(m_ws, 0, (size_t)B * sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_apgd_start_max, apgd_grid(B, quads), dim3(256), 0, st, index, m_ws, quads, seed, restart);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_apgd_start, apgd_grid(B, quads), dim3(256), 0, st, x0, index, m_ws, out, quads, seed, restart, eps, lo, hi);
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
    if (B < 1 || B > 65535 || per_image == 0 || (per_image % 4) || per_image / 4 > 0x7FFFFFFF)
        return nd_set_err(ND_ERR_ARG, "apgd update needs 1 <= B <= 65535 and per_image %% 4 == 0");
    const void* ptrs[] = {x, x_adv, x_adv_old, grad, x_best, grad_best, x_best_adv};
    for (const void* p : ptrs)
        if (!nd_aligned16(p)) return nd_set_err(ND_ERR_ARG, "apgd update needs 16-byte aligned images");
    const int quads = (int)(per_image / 4);
    const dim3 grid = apgd_grid(B, quads);
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
