// nd_vit_grad.hip -- the input gradient of the full ViT (timm 0.4.12 VisionTransformer.forward, cross-entropy on the head): what foolbox's
// LinfBaseGradientDescent asks of the model the reference attacks (attack.py; classification_train_separately.py:661-667,
// utils.py:258-269).  The attack steps built on it are in nd_attack_linf.hip, nd_attack_l2.hip and nd_square.hip.  gfx950 only, all
// arithmetic fp32.
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
#include "nd_math.hpp"
#include "nd_device.hpp"
#include "nd_b9.hpp"
#include "nd_host.hpp"
#include "nd_vit.hpp"

// Every product below is rounded to fp32 before it is used: no contraction into a following add (in particular not into the first
// subtraction of nd_b9_split, which would make a frag32b3 image differ from the split of the fp32 value stored beside it).
#pragma clang fp contract(off)

// ---------------------------------------------------------------------------------------------
// LayerNorm backward, one wave per row: dx = rstd * (gg - mean(gg) - xh * mean(gg * xh)) (+ res), gg = g * gamma, xh = (x - mean) * rstd.
// The statistics are recomputed exactly as k_layernorm (nd_layernorm.hip) computes them (nd_ln_stats).
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
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" int nd_layernorm_bwd(const float* x, const float* gamma, const float* g, const float* residual, float* out, void* out_split,
                                int rows, int dim, float eps, void* stream) {
    if (!x || !gamma || !g || (!out && !out_split)) return nd_set_err(ND_ERR_ARG, "NULL tensor");
    if (rows < 1 || dim < 4 || (dim % 4) || dim > 2048) return nd_set_err(ND_ERR_ARG, "layernorm_bwd needs dim %% 4 == 0, 4 <= dim <= 2048");
    if (out_split && (dim % 32)) return nd_set_err(ND_ERR_ARG, "a split (frag32b3) output needs dim %% 32 == 0");
    const int vpl = (dim + 255) / 256;
    const dim3 grid((rows + 3) / 4), block(256);
    hipStream_t st = (hipStream_t)stream;
    bf16x8* os = reinterpret_cast<bf16x8*>(out_split);
#define LNB_LAUNCH(V) hipLaunchKernelGGL((k_layernorm_bwd<V>), grid, block, 0, st, x, gamma, g, residual, out, os, rows, dim, eps)
    ND_DISPATCH_VPL(vpl, LNB_LAUNCH);
#undef LNB_LAUNCH
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

static int gelu_any(const float* u, const float* dg, float* out, void* out_split, int rows, int cols, bool bwd, void* stream) {
    if (!u || !out_split || (bwd && !dg)) return nd_set_err(ND_ERR_ARG, "NULL tensor");
    if (rows < 1 || cols < 32 || (cols % 32)) return nd_set_err(ND_ERR_ARG, "gelu images need cols %% 32 == 0 (cols=%d)", cols);
    const dim3 grid = nd_b9_image_grid(rows, cols);
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
    hipLaunchKernelGGL(k_unpatchify, dim3(nd_blocks_per_image(total4, 8192)), dim3(256), 0, (hipStream_t)stream, cols, img, B, Cin, Himg, Wimg, p);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}
