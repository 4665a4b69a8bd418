// nd_patchify.hip -- im2col of the ViT's patch embedding (timm 0.4.12 PatchEmbed.proj as a GEMM over patch rows), as fp32 rows
// (nd_patchify) or as the frag32b3 image the patch-embedding GEMM reads (nd_patchify_split).  gfx950 only.  The inverse, nd_unpatchify,
// is in nd_vit_grad.hip.
#include "nd_b9.hpp"
#include "nd_host.hpp"

// ---------------------------------------------------------------------------------------------
// im2col for Conv2d(k = p, stride = p): cols[(b, py, px)][c*p*p + iy*p + ix] = img[b][c][py*p+iy][px*p+ix]
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_patchify(const float* __restrict__ img, float* __restrict__ cols, int B, int Cin,
                                                  int Himg, int Wimg, int p, int split_out) {
    const int gw = Wimg / p, gh = Himg / p;
    const size_t rowlen = (size_t)Cin * p * p;
    const size_t total4 = (size_t)B * gh * gw * rowlen / 4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (size_t)gridDim.x * blockDim.x) {
        const size_t e = i * 4;
        const size_t tok = e / rowlen;
        const int col = (int)(e % rowlen);
        const int c = col / (p * p), iy = (col / p) % p, ix = col % p;
        const int b = (int)(tok / (gh * gw)), py = (int)(tok % (gh * gw)) / gw, px = (int)(tok % gw);
        const float4 v = *reinterpret_cast<const float4*>(img + (((size_t)b * Cin + c) * Himg + (py * p + iy)) * Wimg + px * p + ix);
        if (split_out) nd_b9_store4(reinterpret_cast<bf16x8*>(cols), (int)(rowlen >> 5), (int)tok, col, v.x, v.y, v.z, v.w);
        else *reinterpret_cast<float4*>(cols + e) = v;
    }
}

// im2col -> frag32b3, one wave per (16 tokens x 32 columns) block: a lane gathers the 8 consecutive pixels of its (token, patch row)
// -- 32 contiguous bytes of the image when p % 8 == 0 -- and the wave writes three coalesced 1 KiB planes (the element-wise form
// above scatters 8-byte pieces: 23 us per [32, 3, 224, 224] batch against 12 here).
__global__ __launch_bounds__(256) void k_patchify_split(const float* __restrict__ img, bf16x8* __restrict__ out, int B, int Cin, int Himg, int Wimg,
                                                        int p) {
    const int lane = threadIdx.x & 63;
    const long blk = ((long)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int gw = Wimg / p, gh = Himg / p, rowlen = Cin * p * p, nkb = rowlen >> 5;
    const int R = B * gh * gw;
    if (blk >= (long)((R + 15) >> 4) * nkb) return;
    const int rb = (int)(blk / nkb), kb = (int)(blk - (long)rb * nkb);
    const int tok = rb * 16 + (lane & 15), col = kb * 32 + 8 * (lane >> 4);
    float v[8];
    if (tok < R) {
        const int c = col / (p * p), iy = (col / p) % p, ix = col % p;
        const int b = tok / (gh * gw), py = (tok % (gh * gw)) / gw, px = tok % gw;
        const float* q = img + (((size_t)b * Cin + c) * Himg + (py * p + iy)) * Wimg + px * p + ix;
        const float4 u0 = *reinterpret_cast<const float4*>(q), u1 = *reinterpret_cast<const float4*>(q + 4);
        v[0] = u0.x; v[1] = u0.y; v[2] = u0.z; v[3] = u0.w; v[4] = u1.x; v[5] = u1.y; v[6] = u1.z; v[7] = u1.w;
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = 0.f;
    }
    bf16x8 h1, h2, h3;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        __bf16 a, b2, c2;
        nd_b9_split(v[e], a, b2, c2);
        h1[e] = a; h2[e] = b2; h3[e] = c2;
    }
    out[(blk * 3 + 0) * 64 + lane] = h1;
    out[(blk * 3 + 1) * 64 + lane] = h2;
    out[(blk * 3 + 2) * 64 + lane] = h3;
}

static int patchify_any(const float* img, float* cols, int B, int Cin, int Himg, int Wimg, int p, int split_out, void* stream) {
    if (!img || !cols) return nd_set_err(ND_ERR_ARG, "NULL tensor");
    if (B < 1 || Cin < 1 || p < 4 || (p % 4) || Himg % p || Wimg % p || (Wimg % 4))
        return nd_set_err(ND_ERR_ARG, "patch size must be a multiple of 4 dividing the image");
    if (split_out && ((Cin * p * p) % 32)) return nd_set_err(ND_ERR_ARG, "a split (frag32b3) output needs Cin*p*p %% 32 == 0");
    if (split_out && (p % 8) == 0) {
        hipLaunchKernelGGL(k_patchify_split, nd_b9_image_grid(B * (Himg / p) * (Wimg / p), Cin * p * p), dim3(256), 0, (hipStream_t)stream, img,
                           reinterpret_cast<bf16x8*>(cols), B, Cin, Himg, Wimg, p);
        HIP_CHECK(hipGetLastError());
        return ND_OK;
    }
    const size_t total4 = (size_t)B * Cin * Himg * Wimg / 4;
    hipLaunchKernelGGL(k_patchify, dim3(nd_blocks_per_image(total4, 4096)), dim3(256), 0, (hipStream_t)stream, img, cols, B, Cin, Himg, Wimg, p, split_out);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_patchify(const float* img, float* cols, int B, int Cin, int Himg, int Wimg, int p, void* stream) {
    return patchify_any(img, cols, B, Cin, Himg, Wimg, p, 0, stream);
}

// the same im2col written as the frag32b3 image of [B*(Himg/p)*(Wimg/p), Cin*p*p]: the input of the patch-embedding nd_gemm_split
extern "C" int nd_patchify_split(const float* img, void* cols_split, int B, int Cin, int Himg, int Wimg, int p, void* stream) {
    return patchify_any(img, (float*)cols_split, B, Cin, Himg, Wimg, p, 1, stream);
}
