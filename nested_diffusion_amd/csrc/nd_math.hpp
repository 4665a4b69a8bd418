// nd_math.hpp -- the device arithmetic every kernel family of libnd_hip.so shares: the vector typedefs, the pinned-sequence softplus, the
// LayerNorm row statistics, exp / erf and the activation switch.  Device-only inline code (gfx950 / CDNA4 only); the operation orders
// below are pinned so that every kernel that evaluates one of these returns the same bits for the same argument.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/nested_diffusion.h"      // ND_ACT_*

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float nd_softplus(float x) {
    // torch softplus(beta=1, threshold=20): x if x > 20 else log1p(exp(x)).
    // Evaluated as max(x,0) + log1p(u), u = exp(-|x|) in (0,1], with the compensated form
    // log1p(u) = log(w) - ((w-1)-u)/w, w = fl(1+u)  (1-2 ulp; the correction term is ~1e-8, so an approximate reciprocal
    // is enough).  Half the instructions of log1pf(expf(x)) (whose log1pf goes through f64 here) -- this function is the
    // bulk of the step kernels' epilogue, which runs on one wave per SIMD with nothing to overlap it.
    // The operation sequence is pinned (no contraction left to the compiler, the one FMA explicit): every kernel that evaluates it
    // returns the same bits for the same argument.
#pragma clang fp contract(off)
    const float u = expf(-fabsf(x));
    const float w = 1.0f + u;
    const float c = (w - 1.0f) - u;
    const float r = fmaxf(x, 0.0f) + __builtin_fmaf(-c, __builtin_amdgcn_rcpf(w), logf(w));
    return x > 20.0f ? x : r;
}

// LayerNorm statistics of one row held by a wave (float4 v[i] at column (i * 64 + lane) * 4; entries past dim are zeros): the two-pass
// mean and centred variance, output ((x - mean) - c) * rstd * gamma + beta.  c = sum(x - mean) / dim is the part of the true mean the
// rounded fp32 mean misses; a rounded mean is off by up to half an ulp of |mean|, which a constant row turned into +-ulp * rstd
// (rstd = eps^-1/2 = 1000) instead of 0, and a row of mean 1e4 and spread 1e-2 into a shift of 5 % of its spread.  c is applied (with
// var = (sum (x - mean)^2 - c * sum(x - mean)) / dim) only where it matters -- |c| * rstd > 2^-18, or a variance below eps -- and is 0
// elsewhere: a row below both thresholds keeps the plain two-pass values bit for bit (95-99 % of randn * 3 + 1 rows; the others move by
// an ulp or two).  c and rstd are wave-uniform (butterfly sums).
template <int VPL>
__device__ __forceinline__ void nd_ln_stats(const float4 (&v)[VPL], int lane, int dim, float eps, float& mean, float& c, float& rstd) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    mean = s / (float)dim;
    float sd = 0.f, q = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        if ((i * 64 + lane) * 4 < dim) {
            const float a = v[i].x - mean, b = v[i].y - mean, cc = v[i].z - mean, d = v[i].w - mean;
            q += (a * a + b * b) + (cc * cc + d * d);
            sd += (a + b) + (cc + d);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        q += __shfl_xor(q, off, 64);
        sd += __shfl_xor(sd, off, 64);
    }
    rstd = 1.0f / sqrtf(q / (float)dim + eps);
    c = sd / (float)dim;
    if (fabsf(c) * rstd > 0x1p-18f || q / (float)dim < eps) rstd = 1.0f / sqrtf(fmaxf(__builtin_fmaf(-sd, c, q), 0.f) / (float)dim + eps);
    else c = 0.f;
}

// exp(x) for x <= 0 (softmax arguments), ~1 ulp: exp2 of the product x*log2(e) carried in two pieces (t rounded + its exact
// residual + the low part of log2 e), first-order correction on the result.  v_exp_f32 is the only transcendental; no range
// handling is needed below zero (underflow flushes to 0, as the softmax wants).  x must be finite.
__device__ __forceinline__ float nd_exp_neg(float x) {
    const float L2E = 1.44269504088896340736f, L2E_LO = 1.92596299e-8f, LN2 = 0.69314718055994530942f;
    const float t = x * L2E;
    const float r = __builtin_fmaf(x, L2E, -t) + x * L2E_LO;
    const float p = __builtin_amdgcn_exp2f(t);
    return __builtin_fmaf(p, r * LN2, p);
}

// erf(a) to < 1 ulp of the exact value (measured against fp64 over [-6, 6] with a correctly rounded exp: 0.97 ulp; the device exp above adds
// at most 1 ulp of exp(r) <= 0.4 to the tail branch), branch-free: both of N. Juffa's minimax forms (|a| <= 0.9277: a + a P(a^2); beyond:
// 1 - exp(Q(|a|))) are evaluated and one is selected -- 15 FMAs and one v_exp_f32 per value, where the library erff takes a data-dependent
// branch per lane group.  Used by the exact-erf GELU of timm's Mlp (the fc1 epilogue: 19 M values per ViT block at B = 32).
__device__ __forceinline__ float nd_erf(float a) {
    const float t = fabsf(a), s = a * a;
    float r = __builtin_fmaf(-1.72853470e-5f, t, 3.83197126e-4f);
    const float u = __builtin_fmaf(-3.88396438e-3f, t, 2.42546219e-2f);
    r = __builtin_fmaf(r, s, u);
    r = __builtin_fmaf(r, t, -1.06777877e-1f);
    r = __builtin_fmaf(r, t, -6.34846687e-1f);
    r = __builtin_fmaf(r, t, -1.28717512e-1f);
    r = __builtin_fmaf(r, t, -t);
    const float big = __builtin_copysignf(1.0f - nd_exp_neg(fmaxf(r, -100.0f)), a);      // (the clamp keeps the argument finite for huge |a|)
    float q = -5.96761703e-4f;
    q = __builtin_fmaf(q, s, 4.99119423e-3f);
    q = __builtin_fmaf(q, s, -2.67681349e-2f);
    q = __builtin_fmaf(q, s, 1.12819925e-1f);
    q = __builtin_fmaf(q, s, -3.76125336e-1f);
    q = __builtin_fmaf(q, s, 1.28379166e-1f);
    const float small = __builtin_fmaf(q, a, a);
    return t > 0.927734375f ? big : small;
}

__device__ __forceinline__ float nd_act(float v, int act) {
    switch (act) {
        case ND_ACT_SOFTPLUS: return nd_softplus(v);
        case ND_ACT_RELU: return v > 0.0f ? v : 0.0f;
        case ND_ACT_GELU: return 0.5f * v * (1.0f + nd_erf(v * 0.70710678118654752440f));
        default: return v;
    }
}
