// nd_layernorm.hip -- LayerNorm forward of the ViT blocks (timm 0.4.12 Block.norm1 / norm2), with its result as fp32 rows (nd_layernorm)
// or as the frag32b3 image the Linear that follows reads (nd_layernorm_split).  gfx950 only.  The backward is in nd_vit_grad.hip.
#include "nd_math.hpp"
#include "nd_device.hpp"
#include "nd_b9.hpp"
#include "nd_host.hpp"
#include "nd_vit.hpp"

// ---------------------------------------------------------------------------------------------
// LayerNorm over the last dim; one wave per row, two-pass (mean, then centred variance) in registers (nd_ln_stats,
// nd_math.hpp).
// ---------------------------------------------------------------------------------------------
// SPLIT: the result is written as a frag32b3 image (csrc/nd_b9.hpp) -- the input form of the Linear layer that follows every
// LayerNorm of a ViT block -- instead of fp32 row-major: a lane's 4 consecutive columns are three 8-byte pieces.
template <int VPL, bool SPLIT>  // float4 per lane: dim <= 64*4*VPL
__global__ __launch_bounds__(256) void k_layernorm(const float* __restrict__ x, const float* __restrict__ gamma,
                                                   const float* __restrict__ beta, float* __restrict__ out, int rows, int dim,
                                                   float eps) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* p = x + (size_t)row * dim;
    float4 v[VPL];
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int c = (i * 64 + lane) * 4;
        v[i] = c < dim ? *reinterpret_cast<const float4*>(p + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float mean, cm, rstd;
    nd_ln_stats<VPL>(v, lane, dim, eps, mean, cm, rstd);
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (c < dim) {
            const float4 g = *reinterpret_cast<const float4*>(gamma + c);
            const float4 b = *reinterpret_cast<const float4*>(beta + c);
            float4 o;
            o.x = ((v[i].x - mean) - cm) * rstd * g.x + b.x;
            o.y = ((v[i].y - mean) - cm) * rstd * g.y + b.y;
            o.z = ((v[i].z - mean) - cm) * rstd * g.z + b.z;
            o.w = ((v[i].w - mean) - cm) * rstd * g.w + b.w;
            if (SPLIT) nd_b9_store4(reinterpret_cast<bf16x8*>(out), dim >> 5, row, c, o.x, o.y, o.z, o.w);
            else *reinterpret_cast<float4*>(out + (size_t)row * dim + c) = o;
        }
    }
}

// LayerNorm -> frag32b3 for 16 rows per workgroup (16 waves, one row each): the pieces are gathered in LDS as the block-row's image --
// which is ONE contiguous run of (dim/32) * 3 KiB in global memory -- and copied out in coalesced 16-byte units.  (The direct form
// above scatters 8-byte pieces 256 bytes apart: ~15 us per [6272, 768] launch; this one 13.5 us against 8.1 us for the fp32 LayerNorm
// and a floor of ~10 us for 19 MB read + 29 MB written; with 4 waves x 4 rows per workgroup it took 18 us: a row is two dependent
// shuffle reductions, four of them in a row are a latency chain.  tools/bench_ln_split.py)
template <int VPL>
__global__ __launch_bounds__(1024) void k_layernorm_split16(const float* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, bf16x8* __restrict__ out, int rows, int dim, float eps) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ln_img[];      // [dim/32][3][64][16 B]
    const int lane = threadIdx.x & 63, r16 = threadIdx.x >> 6;
    const int nkb = dim >> 5;
    {
        const int row = blockIdx.x * 16 + r16;
        float4 v[VPL];
        const bool live = row < rows;
        const float* p = x + (size_t)(live ? row : 0) * dim;
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
            const int c = (i * 64 + lane) * 4;
            v[i] = (live && c < dim) ? *reinterpret_cast<const float4*>(p + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        float mean, cm, rstd;
        nd_ln_stats<VPL>(v, lane, dim, eps, mean, cm, rstd);
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
            const int c = (i * 64 + lane) * 4;
            if (c < dim) {
                const float4 g = *reinterpret_cast<const float4*>(gamma + c);
                const float4 b = *reinterpret_cast<const float4*>(beta + c);
                float o[4];
                o[0] = live ? ((v[i].x - mean) - cm) * rstd * g.x + b.x : 0.f;
                o[1] = live ? ((v[i].y - mean) - cm) * rstd * g.y + b.y : 0.f;
                o[2] = live ? ((v[i].z - mean) - cm) * rstd * g.z + b.z : 0.f;
                o[3] = live ? ((v[i].w - mean) - cm) * rstd * g.w + b.w : 0.f;
                bf16x4 p1, p2, p3;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    __bf16 h1, h2, h3;
                    nd_b9_split(o[e], h1, h2, h3);
                    p1[e] = h1; p2[e] = h2; p3[e] = h3;
                }
                unsigned char* q8 = ln_img + (size_t)(c >> 5) * 3072 + (r16 + 16 * ((c & 31) >> 3)) * 16 + ((c & 7) >> 2) * 8;
                *reinterpret_cast<bf16x4*>(q8) = p1;
                *reinterpret_cast<bf16x4*>(q8 + 1024) = p2;
                *reinterpret_cast<bf16x4*>(q8 + 2048) = p3;
            }
        }
    }
    __syncthreads();
    const uint4* src = reinterpret_cast<const uint4*>(ln_img);
    uint4* dst = reinterpret_cast<uint4*>(out + (size_t)blockIdx.x * nkb * B9_BLOCK_UNITS);
    for (int i = threadIdx.x; i < nkb * B9_BLOCK_UNITS; i += 1024) dst[i] = src[i];
}

template <bool SPLIT>
static int launch_layernorm(const float* x, const float* gamma, const float* beta, float* out, int rows, int dim, float eps, void* stream) {
    if (!x || !gamma || !beta || !out) return nd_set_err(ND_ERR_ARG, "NULL tensor");
    if (rows < 1 || dim < 4 || (dim % 4) || dim > 64 * 4 * 8) return nd_set_err(ND_ERR_ARG, "dim must be a multiple of 4 in [4,2048]");
    if (SPLIT && (dim % 32)) return nd_set_err(ND_ERR_ARG, "a split (frag32b3) output needs dim %% 32 == 0 (dim=%d)", dim);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((rows + 3) / 4), block(256);
    const int vpl = (dim + 255) / 256;
    if (SPLIT && rows >= 64 && dim <= 1024) {
        // 16 rows per workgroup through an LDS image (<= 96 KiB): coalesced stores
        const dim3 g16((rows + 15) / 16);
        const size_t lds = (size_t)(dim / 32) * 3072;
        bf16x8* img = reinterpret_cast<bf16x8*>(out);
#define LN16(V)                                                                                                                      \
        {                                                                                                                            \
            HIP_CHECK(nd_allow_dynamic_lds((const void*)k_layernorm_split16<V>, 96 * 1024));                                         \
            hipLaunchKernelGGL((k_layernorm_split16<V>), g16, dim3(1024), lds, st, x, gamma, beta, img, rows, dim, eps);                  \
        }
        if (vpl <= 1) LN16(1) else if (vpl <= 2) LN16(2) else if (vpl <= 3) LN16(3) else LN16(4)
#undef LN16
        HIP_CHECK(hipGetLastError());
        return ND_OK;
    }
#define LN_LAUNCH(V) hipLaunchKernelGGL((k_layernorm<V, SPLIT>), grid, block, 0, st, x, gamma, beta, out, rows, dim, eps)
    ND_DISPATCH_VPL(vpl, LN_LAUNCH);
#undef LN_LAUNCH
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_layernorm(const float* x, const float* gamma, const float* beta, float* out, int rows, int dim, float eps,
                            void* stream) {
    return launch_layernorm<false>(x, gamma, beta, out, rows, dim, eps, stream);
}

// the same LayerNorm with its result written as the frag32b3 image of [rows, dim] (dim % 32 == 0): the input of nd_gemm_split
extern "C" int nd_layernorm_split(const float* x, const float* gamma, const float* beta, void* out_split, int rows, int dim, float eps,
                                  void* stream) {
    return launch_layernorm<true>(x, gamma, beta, (float*)out_split, rows, dim, eps, stream);
}
