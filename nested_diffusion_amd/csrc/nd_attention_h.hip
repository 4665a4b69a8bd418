// nd_attention_h.hip -- the fp16-operand attention core of the ViT blocks (the fp16 mode; head dim 64), behind nd_launch_attention_h.
// gfx950 only.  A unit of its own: the fp32 kernels of nd_attention.hip are built with -mllvm -amdgpu-mfma-vgpr-form, this one is not.
// Entry points and the MFMA operand maps it shares with the RING kernel: nd_attention.hip.
#include "nd_math.hpp"
#include "nd_device.hpp"
#include "nd_vit.hpp"

// fp16-operand form (the fp16 mode; not a mode of the reference): q, k, v are rounded to fp16 as they are staged, both
// contractions run on v_mfma_f32_16x16x32_f16 with fp32 accumulation, the softmax is fp32 and the normalised probabilities
// are rounded to fp16 for the second contraction.  K is staged row-major [key][64+8] (a lane's 8 halfs d = 8g..+7 of key
// l&15: one ds_read_b128), V TRANSPOSED [d][keys+8] so that the 8 k-slots of a lane are two runs of 4 consecutive keys
// {32F+4g..+3} and {32F+16+4g..+3} -- exactly the keys whose scores that lane already holds in the accumulators of score
// fragments 2F and 2F+1 (D[i=4g+r][j=query]), so P needs no cross-lane movement.
#define AH_KLD 72
template <int NF>
__global__ __launch_bounds__(NF * 64) void k_attention_h(const float* __restrict__ qkv, float* __restrict__ out, int B, int N,
                                                          int heads) {
    constexpr int NFP = (NF + 1) / 2 * 2;                 // score fragments, padded to pairs
    constexpr int VLD = 16 * NFP + 8;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    _Float16* sK = reinterpret_cast<_Float16*>(smem);     // [16*NFP][AH_KLD]
    _Float16* sVt = sK + 16 * NFP * AH_KLD;               // [64][VLD]
    const int tid = threadIdx.x, lane = tid & 63, wave = blockIdx.y * (blockDim.x >> 6) + (tid >> 6);
    const int bh = blockIdx.x, b = bh / heads, hd = bh % heads;
    const int Cm = heads * 64;
    const size_t rs = (size_t)3 * Cm;
    const float* base = qkv + (size_t)b * N * rs + (size_t)hd * 64;
    const float* qb = base;
    const float* kb = base + Cm;
    const float* vb = base + 2 * Cm;
    for (int e0 = tid; e0 < 16 * NFP * 16; e0 += 4 * blockDim.x) {     // 16 float4 per 64-float row
        float4 k4[4], v4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = e0 + u * blockDim.x, row = e >> 4, c4 = (e & 15) * 4;
            k4[u] = make_float4(0.f, 0.f, 0.f, 0.f); v4[u] = k4[u];
            if (e < 16 * NFP * 16 && row < N) {
                k4[u] = *reinterpret_cast<const float4*>(kb + (size_t)row * rs + c4);
                v4[u] = *reinterpret_cast<const float4*>(vb + (size_t)row * rs + c4);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = e0 + u * blockDim.x, row = e >> 4, c4 = (e & 15) * 4;
            if (e < 16 * NFP * 16) {
                *reinterpret_cast<f16x4*>(sK + row * AH_KLD + c4) = f16x4{(_Float16)k4[u].x, (_Float16)k4[u].y, (_Float16)k4[u].z, (_Float16)k4[u].w};
                sVt[(c4 + 0) * VLD + row] = (_Float16)v4[u].x;
                sVt[(c4 + 1) * VLD + row] = (_Float16)v4[u].y;
                sVt[(c4 + 2) * VLD + row] = (_Float16)v4[u].z;
                sVt[(c4 + 3) * VLD + row] = (_Float16)v4[u].w;
            }
        }
    }
    const int g = lane >> 4, li = lane & 15;
    const int qrow = min(wave * 16 + li, N - 1);
    f16x8 qh[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float4 a = *reinterpret_cast<const float4*>(qb + (size_t)qrow * rs + 32 * c + 8 * g);
        const float4 bq = *reinterpret_cast<const float4*>(qb + (size_t)qrow * rs + 32 * c + 8 * g + 4);
        qh[c] = f16x8{(_Float16)a.x, (_Float16)a.y, (_Float16)a.z, (_Float16)a.w, (_Float16)bq.x, (_Float16)bq.y, (_Float16)bq.z, (_Float16)bq.w};
    }
    __syncthreads();
    f32x4 s[NFP];
#pragma unroll
    for (int f = 0; f < NFP; ++f) {
        s[f] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const f16x8 kv = *reinterpret_cast<const f16x8*>(sK + (16 * f + li) * AH_KLD + 32 * c + 8 * g);
            s[f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kv, qh[c], s[f], 0, 0, 0);      // D[i = key 4g+r][j = query li]
        }
    }
    const float scale = 0.125f;  // 64^-0.5
    float mx = -INFINITY;
#pragma unroll
    for (int f = 0; f < NFP; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int key = 16 * f + 4 * g + r;
            const float v = key < N ? s[f][r] * scale : -INFINITY;
            s[f][r] = v;
            mx = fmaxf(mx, v);
        }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float sum = 0.f;
#pragma unroll
    for (int f = 0; f < NFP; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float p = expf(s[f][r] - mx);
            s[f][r] = p;
            sum += p;
        }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.0f / sum;
    f32x4 o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int F2 = 0; F2 < NFP / 2; ++F2) {
        const f16x8 ph = {(_Float16)(s[2 * F2][0] * inv), (_Float16)(s[2 * F2][1] * inv), (_Float16)(s[2 * F2][2] * inv), (_Float16)(s[2 * F2][3] * inv),
                          (_Float16)(s[2 * F2 + 1][0] * inv), (_Float16)(s[2 * F2 + 1][1] * inv), (_Float16)(s[2 * F2 + 1][2] * inv),
                          (_Float16)(s[2 * F2 + 1][3] * inv)};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const _Float16* vp = sVt + (16 * e + li) * VLD + 32 * F2 + 4 * g;
            const f16x4 v0 = *reinterpret_cast<const f16x4*>(vp), v1 = *reinterpret_cast<const f16x4*>(vp + 16);
            const f16x8 vh = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
            o[e] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh, ph, o[e], 0, 0, 0);          // D[i = d 16e+4g+r][j = query li]
        }
    }
    const int qo = wave * 16 + li;
    if (qo < N) {
        float* op = out + ((size_t)b * N + qo) * Cm + (size_t)hd * 64 + 4 * g;
#pragma unroll
        for (int e = 0; e < 4; ++e) *reinterpret_cast<float4*>(op + 16 * e) = make_float4(o[e][0], o[e][1], o[e][2], o[e][3]);
    }
}

template <int NF>
static hipError_t launch_attention_h(const float* qkv, float* out, int B, int N, int heads, hipStream_t st) {
    constexpr int NFP = (NF + 1) / 2 * 2;
    const size_t lds = ((size_t)16 * NFP * AH_KLD + (size_t)64 * (16 * NFP + 8)) * sizeof(_Float16);
    {
        hipError_t e = nd_allow_dynamic_lds((const void*)k_attention_h<NF>, lds);
        if (e != hipSuccess) return e;
    }
    int qs = 1;
    while (qs < 4 && (long)B * heads * qs < 768 && (NF + qs) / (qs + 1) >= 2) ++qs;
    if (qs > NF) qs = NF;
    const int wpq = (NF + qs - 1) / qs;
    hipLaunchKernelGGL((k_attention_h<NF>), dim3(B * heads, (NF + wpq - 1) / wpq), dim3(wpq * 64), lds, st, qkv, out, B, N, heads);
    return hipGetLastError();
}

hipError_t nd_launch_attention_h(const float* qkv, float* out, int B, int N, int heads, hipStream_t st) {
#define AH_LAUNCH(NFV) return launch_attention_h<NFV>(qkv, out, B, N, heads, st)
    ND_DISPATCH_NF((N + 15) / 16, AH_LAUNCH)
#undef AH_LAUNCH
    return hipErrorInvalidValue;
}
