// nd_image.hip -- input-side perturbations of the robustness protocol (diffusion/utils.py:272-414, applied at
// classification_train_separately.py:726-737): elementwise / resampling kernels on [B, C, H, W] fp32 images; and the batch
// gather of the training input (a device-resident uint8 image store -> one fp32 batch).  gfx950 only.
#include "nd_host.hpp"

static inline dim3 grid1(size_t n, int per = 256) {
    const size_t b = (n + per - 1) / per;
    return dim3((unsigned)(b > 65535 * 16 ? 65535 * 16 : (b ? b : 1)));
}

// out = x + z * std           (add_noise, utils.py:272-279; z = the torch.randn_like draw, supplied)
__global__ void k_add_noise(const float* __restrict__ x, const float* __restrict__ z, float* __restrict__ out, size_t n, float std_) {
#pragma clang fp contract(off)
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) out[i] = x[i] + z[i] * std_;
}
// out = clamp(x + k, 0, 1)    (adjust_brightness, utils.py:390-399)
__global__ void k_brightness(const float* __restrict__ x, float* __restrict__ out, size_t n, float k) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        out[i] = fminf(fmaxf(x[i] + k, 0.f), 1.f);
}
// per-image mean over C*H*W (adjust_contrast, utils.py:405-406): one workgroup per image, fixed reduction tree
__global__ __launch_bounds__(1024) void k_image_mean(const float* __restrict__ x, float* __restrict__ mean, size_t per) {
    const float* p = x + (size_t)blockIdx.x * per;
    float s = 0.f;
    for (size_t i = threadIdx.x; i < per; i += 1024) s += p[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    __shared__ float red[16];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int w = 0; w < 16; ++w) t += red[w];
        mean[blockIdx.x] = t / (float)per;
    }
}
// out = clamp(mean + (x - mean) * k, 0, 1)   (utils.py:408-412)
__global__ void k_contrast(const float* __restrict__ x, const float* __restrict__ mean, float* __restrict__ out, size_t per, size_t n, float k) {
#pragma clang fp contract(off)
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float m = mean[i / per];
        out[i] = fminf(fmaxf(m + (x[i] - m) * k, 0.f), 1.f);
    }
}

// Bilinear resize, torch.nn.functional.interpolate(mode='bilinear', align_corners=False, no antialias) semantics:
// src = max(scale * (dst + 0.5) - 0.5, 0), scale = in / out; neighbours clamped at the border.  The source coordinate is ONE fused
// multiply-add, as torch's builds compute it (their compilers contract the expression): rounding the product first moves a weight
// by up to an ulp of the coordinate, 4e-7 of the result when 7 x 9 is resized to 224 x 224.  The blend stays uncontracted.
// Optional per-image crop window (top, left, size x size) read from `crop` (random_crop_and_resize, utils.py:282-312).
__global__ void k_resize_bilinear(const float* __restrict__ x, float* __restrict__ out, int NC, int C, int Hi, int Wi, int Ho, int Wo,
                                  const int* __restrict__ crop, int crop_size) {
#pragma clang fp contract(off)
    const size_t total = (size_t)NC * Ho * Wo;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int ox = (int)(i % Wo), oy = (int)((i / Wo) % Ho), nc = (int)(i / ((size_t)Wo * Ho));
        int top = 0, left = 0, hi = Hi, wi = Wi;
        if (crop) { const int b = nc / C; top = crop[2 * b]; left = crop[2 * b + 1]; hi = crop_size; wi = crop_size; }
        const float sh = (float)hi / (float)Ho, sw = (float)wi / (float)Wo;
        const float fy = fmaxf(fmaf(sh, (float)oy + 0.5f, -0.5f), 0.f), fx = fmaxf(fmaf(sw, (float)ox + 0.5f, -0.5f), 0.f);
        const int y0 = min((int)fy, hi - 1), x0 = min((int)fx, wi - 1);
        const int y1 = y0 + (y0 < hi - 1 ? 1 : 0), x1 = x0 + (x0 < wi - 1 ? 1 : 0);
        const float ly = fy - (float)y0, lx = fx - (float)x0, hy = 1.f - ly, hx = 1.f - lx;
        const float* p = x + (size_t)nc * Hi * Wi;
        const float v00 = p[(size_t)(top + y0) * Wi + left + x0], v01 = p[(size_t)(top + y0) * Wi + left + x1];
        const float v10 = p[(size_t)(top + y1) * Wi + left + x0], v11 = p[(size_t)(top + y1) * Wi + left + x1];
        out[i] = hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11);
    }
}

// zero `n_rects` squares of side `side` per image (random_cover_new, utils.py:315-349); rects[b][r] = (top, left)
__global__ void k_cover(float* __restrict__ x, int B, int C, int H, int W, const int* __restrict__ rects, int n_rects, int side) {
    const size_t per = (size_t)n_rects * C * side * side, total = (size_t)B * per;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int dx = (int)(i % side), dy = (int)((i / side) % side), c = (int)((i / ((size_t)side * side)) % C);
        const int r = (int)((i / ((size_t)side * side * C)) % n_rects), b = (int)(i / per);
        const int top = rects[((size_t)b * n_rects + r) * 2], left = rects[((size_t)b * n_rects + r) * 2 + 1];
        x[(((size_t)b * C + c) * H + top + dy) * W + left + dx] = 0.f;
    }
}

// Training input: out[b][c][p] = lut[c][store[idx[b]][Cs == 1 ? 0 : c][p]] -- one batch formed from the device-resident uint8 store.
// The byte -> float transform is the 3 x 256 table (staged in LDS once per workgroup), so no arithmetic touches a value.  Workgroups
// (x, y) walk whole image rows: y the batch rows, x the pixels of one.  VEC: a lane loads 4 bytes per channel and stores one float4
// (pixels % 4 == 0 and 4- / 16-byte aligned bases, decided by the host); otherwise a byte and a float.  Offsets into the store are 64-bit.
// A row whose index is outside [0, n_images) reads nothing and writes nothing (the index lives on the device: the host cannot refuse it).
template <bool VEC>
__global__ __launch_bounds__(256) void k_gather_u8(const uint8_t* __restrict__ store, long long n_images, int Cs, int pixels,
                                                   const int* __restrict__ idx, int B, const float* __restrict__ lut, float* __restrict__ out) {
    __shared__ float t[3 * 256];
    for (int i = threadIdx.x; i < 3 * 256; i += 256) t[i] = lut[i];
    __syncthreads();
    const size_t cstride = Cs == 1 ? 0 : (size_t)pixels;
    const size_t first = (size_t)blockIdx.x * 256 + threadIdx.x, step = (size_t)gridDim.x * 256;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const long long r = idx[b];
        if (r < 0 || r >= n_images) continue;
        const uint8_t* src = store + (size_t)r * (size_t)Cs * (size_t)pixels;
        float* dst = out + (size_t)b * 3 * (size_t)pixels;
        if (VEC) {
            const size_t quads = (size_t)pixels >> 2;
            for (size_t q = first; q < quads; q += step) {
                uint32_t w = 0;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    if (c == 0 || Cs == 3) w = reinterpret_cast<const uint32_t*>(src + c * cstride)[q];
                    const float* tc = t + c * 256;
                    reinterpret_cast<float4*>(dst + (size_t)c * pixels)[q] =
                        make_float4(tc[w & 255u], tc[(w >> 8) & 255u], tc[(w >> 16) & 255u], tc[w >> 24]);
                }
            }
        } else {
            for (size_t p = first; p < (size_t)pixels; p += step)
#pragma unroll
                for (int c = 0; c < 3; ++c) dst[(size_t)c * pixels + p] = t[c * 256 + src[c * cstride + p]];
        }
    }
}

extern "C" int nd_img_add_noise(const float* x, const float* z, float* out, size_t n, float std_, void* stream) {
    if (!x || !z || !out || n == 0) return nd_set_err(ND_ERR_ARG, "bad add_noise arguments");
    hipLaunchKernelGGL(k_add_noise, grid1(n), dim3(256), 0, (hipStream_t)stream, x, z, out, n, std_);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}
extern "C" int nd_img_brightness(const float* x, float* out, size_t n, float k, void* stream) {
    if (!x || !out || n == 0) return nd_set_err(ND_ERR_ARG, "bad brightness arguments");
    hipLaunchKernelGGL(k_brightness, grid1(n), dim3(256), 0, (hipStream_t)stream, x, out, n, k);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}
extern "C" int nd_img_contrast(const float* x, float* out, float* mean_ws, int B, size_t per_image, float k, void* stream) {
    if (!x || !out || !mean_ws) return nd_set_err(ND_ERR_ARG, "contrast: NULL tensor");
    if (B < 1 || per_image == 0) return nd_set_err(ND_ERR_ARG, "contrast needs B >= 1 and per_image >= 1 (B=%d, per_image=%zu)", B, per_image);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_image_mean, dim3(B), dim3(1024), 0, st, x, mean_ws, per_image);
    const size_t n = (size_t)B * per_image;
    hipLaunchKernelGGL(k_contrast, grid1(n), dim3(256), 0, st, x, (const float*)mean_ws, out, per_image, n, k);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}
extern "C" int nd_img_resize_bilinear(const float* x, float* out, int B, int C, int Hi, int Wi, int Ho, int Wo, const int32_t* crop,
                                      int crop_size, void* stream) {
    if (!x || !out) return nd_set_err(ND_ERR_ARG, "resize: NULL tensor");
    if (B < 1 || C < 1 || Hi < 1 || Wi < 1 || Ho < 1 || Wo < 1)
        return nd_set_err(ND_ERR_ARG, "resize needs every size >= 1 (B=%d, C=%d, Hi=%d, Wi=%d, Ho=%d, Wo=%d)", B, C, Hi, Wi, Ho, Wo);
    if (crop && (crop_size < 1 || crop_size > Hi || crop_size > Wi))
        return nd_set_err(ND_ERR_ARG, "need 1 <= crop_size <= min(Hi, Wi) (crop_size=%d, Hi=%d, Wi=%d)", crop_size, Hi, Wi);
    const size_t total = (size_t)B * C * Ho * Wo;
    hipLaunchKernelGGL(k_resize_bilinear, grid1(total), dim3(256), 0, (hipStream_t)stream, x, out, B * C, C, Hi, Wi, Ho, Wo, (const int*)crop, crop_size);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}
extern "C" int nd_img_cover(float* x, int B, int C, int H, int W, const int32_t* rects, int n_rects, int side, void* stream) {
    if (!x || !rects) return nd_set_err(ND_ERR_ARG, "cover: NULL tensor");
    if (B < 1 || C < 1 || n_rects < 1 || side < 0 || side > H || side > W)
        return nd_set_err(ND_ERR_ARG, "cover needs B, C, n_rects >= 1 and 0 <= side <= min(H, W) (B=%d, C=%d, n_rects=%d, side=%d, H=%d, W=%d)", B, C,
                          n_rects, side, H, W);
    if (side == 0) return ND_OK;
    const size_t total = (size_t)B * n_rects * C * side * side;
    hipLaunchKernelGGL(k_cover, grid1(total), dim3(256), 0, (hipStream_t)stream, x, B, C, H, W, (const int*)rects, n_rects, side);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}
extern "C" int nd_img_gather_u8(const uint8_t* store, long long n_images, int src_channels, int pixels, const int32_t* idx, int B,
                                const float* lut, float* out, void* stream) {
    if (!store || !idx || !lut || !out) return nd_set_err(ND_ERR_ARG, "gather_u8: NULL tensor");
    if (src_channels != 1 && src_channels != 3) return nd_set_err(ND_ERR_ARG, "gather_u8 needs src_channels 1 or 3 (src_channels=%d)", src_channels);
    if (pixels < 1 || B < 1 || n_images < 1)
        return nd_set_err(ND_ERR_ARG, "gather_u8 needs pixels, B, n_images >= 1 (pixels=%d, B=%d, n_images=%lld)", pixels, B, n_images);
    if (((uintptr_t)out | (uintptr_t)lut | (uintptr_t)idx) & 3)
        return nd_set_err(ND_ERR_ARG, "gather_u8: out, lut and idx must be 4-byte aligned");
    const bool vec = pixels % 4 == 0 && ((uintptr_t)store & 3) == 0 && ((uintptr_t)out & 15) == 0;
    const size_t per_wg = vec ? 2048 : 512;                          // pixels of a row per workgroup: two passes of its 256 lanes
    const size_t gx = ((size_t)pixels + per_wg - 1) / per_wg;
    const dim3 grid((unsigned)(gx > 65535 ? 65535 : gx), (unsigned)(B > 65535 ? 65535 : B));
    if (vec)
        hipLaunchKernelGGL(k_gather_u8<true>, grid, dim3(256), 0, (hipStream_t)stream, store, n_images, src_channels, pixels, (const int*)idx, B, lut, out);
    else
        hipLaunchKernelGGL(k_gather_u8<false>, grid, dim3(256), 0, (hipStream_t)stream, store, n_images, src_channels, pixels, (const int*)idx, B, lut, out);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}
