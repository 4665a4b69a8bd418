// nd_pack.hip -- row-major <-> frag16 / frag32h (nd_frag.hpp): the four pack / unpack kernels, their two launchers and the entry points
// nd_packed_bytes, nd_pack_rows, nd_unpack_rows (include/nested_diffusion.h).  gfx950 only.
#include "nd_frag.hpp"
#include "nd_host.hpp"

// row-major fp32 [R][K] -> frag32h (round to nearest even); rows R .. 16*ceil(R/16) zero-filled.  16 B per thread.
__global__ __launch_bounds__(256) void k_pack_rows_h(const float* __restrict__ src, _Float16* __restrict__ dst, int R, int K) {
    const int nch = K >> 5;
    const size_t total = (size_t)((R + 15) / 16) * nch * 64;   // 16-byte pieces
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int lane = (int)(i & 63);
        const size_t blk = i >> 6;
        const int rt = (int)(blk / nch), c = (int)(blk % nch);
        const int r = rt * 16 + (lane & 15);
        f16x8 h = {0, 0, 0, 0, 0, 0, 0, 0};
        if (r < R) {
            const float* p = src + (size_t)r * K + c * 32 + 8 * (lane >> 4);
            const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
            h = f16x8{(_Float16)a.x, (_Float16)a.y, (_Float16)a.z, (_Float16)a.w, (_Float16)b.x, (_Float16)b.y, (_Float16)b.z, (_Float16)b.w};
        }
        reinterpret_cast<f16x8*>(dst)[i] = h;
    }
}

// frag32h [R][K] -> row-major fp32 (tests / debugging)
__global__ __launch_bounds__(256) void k_unpack_rows_h(const _Float16* __restrict__ src, float* __restrict__ dst, int R, int K) {
    const int nch = K >> 5;
    const size_t total = (size_t)((R + 15) / 16) * nch * 64;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int lane = (int)(i & 63);
        const size_t blk = i >> 6;
        const int rt = (int)(blk / nch), c = (int)(blk % nch);
        const int r = rt * 16 + (lane & 15);
        if (r < R) {
            const f16x8 h = reinterpret_cast<const f16x8*>(src)[i];
            float* p = dst + (size_t)r * K + c * 32 + 8 * (lane >> 4);
#pragma unroll
            for (int j = 0; j < 8; ++j) p[j] = (float)h[j];
        }
    }
}

// row-major [R][K] -> frag16; rows R .. 16*ceil(R/16) are zero-filled.  One float4 per thread.
__global__ __launch_bounds__(256) void k_pack_rows(const float* __restrict__ src, float* __restrict__ dst, int R, int K) {
    const int nch = K >> 4;
    const size_t total = (size_t)((R + 15) / 16) * nch * 64;   // float4 count
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int lane = (int)(i & 63);
        const size_t blk = i >> 6;
        const int rt = (int)(blk / nch), c = (int)(blk % nch);
        const int r = rt * 16 + (lane & 15);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < R) v = *reinterpret_cast<const float4*>(src + (size_t)r * K + c * 16 + 4 * (lane >> 4));
        reinterpret_cast<float4*>(dst)[i] = v;
    }
}

// frag16 [R][K] -> row-major (tests / debugging)
__global__ __launch_bounds__(256) void k_unpack_rows(const float* __restrict__ src, float* __restrict__ dst, int R, int K) {
    const int nch = K >> 4;
    const size_t total = (size_t)((R + 15) / 16) * nch * 64;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int lane = (int)(i & 63);
        const size_t blk = i >> 6;
        const int rt = (int)(blk / nch), c = (int)(blk % nch);
        const int r = rt * 16 + (lane & 15);
        if (r < R) *reinterpret_cast<float4*>(dst + (size_t)r * K + c * 16 + 4 * (lane >> 4)) = reinterpret_cast<const float4*>(src)[i];
    }
}

// ---- the two launchers ------------------------------------------------------------------------
// One thread per 16-byte piece of the image, at most 8192 workgroups: above that (images over 32 MiB) the kernels' grid-stride loops take
// further trips.  Every piece is written by exactly one thread whatever the grid, so results do not depend on it.
static dim3 pack_grid(int R, int K, int half) {
    const size_t n16 = nd_packed_bytes_dt(R, K, half) / 16, want = (n16 + 255) / 256;
    return dim3((unsigned)(want > 8192 ? 8192 : want));
}

void nd_launch_pack(const float* src, void* dst, int R, int K, int half, hipStream_t st) {
    if (half) hipLaunchKernelGGL(k_pack_rows_h, pack_grid(R, K, 1), dim3(256), 0, st, src, (_Float16*)dst, R, K);
    else hipLaunchKernelGGL(k_pack_rows, pack_grid(R, K, 0), dim3(256), 0, st, src, (float*)dst, R, K);
}

void nd_launch_unpack(const void* src, float* dst, int R, int K, int half, hipStream_t st) {
    if (half) hipLaunchKernelGGL(k_unpack_rows_h, pack_grid(R, K, 1), dim3(256), 0, st, (const _Float16*)src, dst, R, K);
    else hipLaunchKernelGGL(k_unpack_rows, pack_grid(R, K, 0), dim3(256), 0, st, (const float*)src, dst, R, K);
}

// ---- entry points -----------------------------------------------------------------------------
static int bad_dtype(int dtype) { return dtype != ND_DTYPE_F32 && dtype != ND_DTYPE_F16; }
static int kmul(int dtype) { return dtype == ND_DTYPE_F16 ? 32 : 16; }

extern "C" size_t nd_packed_bytes(int R, int K, int dtype) {
    if (bad_dtype(dtype) || R < 1 || K < kmul(dtype) || (K % kmul(dtype))) return 0;
    return nd_packed_bytes_dt(R, K, dtype == ND_DTYPE_F16);
}

extern "C" int nd_pack_rows(const float* src, void* dst, int R, int K, int dtype, void* stream) {
    if (!src || !dst) return nd_set_err(ND_ERR_ARG, "NULL tensor");
    if (bad_dtype(dtype)) return nd_set_err(ND_ERR_ARG, "unknown dtype %d", dtype);
    if (R < 1 || K < kmul(dtype) || (K % kmul(dtype)))
        return nd_set_err(ND_ERR_ARG, "need R >= 1 and K a positive multiple of %d (K=%d)", kmul(dtype), K);
    nd_launch_pack(src, dst, R, K, dtype == ND_DTYPE_F16, (hipStream_t)stream);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_unpack_rows(const void* src_packed, float* dst, int R, int K, int dtype, void* stream) {
    if (!src_packed) return nd_set_err(ND_ERR_ARG, "unpack_rows: NULL image src_packed");
    if (!dst) return nd_set_err(ND_ERR_ARG, "unpack_rows: NULL tensor dst");
    if (dtype != ND_DTYPE_F32) return nd_set_err(ND_ERR_ARG, "unpack_rows: dtype must be ND_DTYPE_F32: only fp32 (frag16) images are unpacked");
    if (R < 1 || K < 16 || K % 16) return nd_set_err(ND_ERR_ARG, "unpack_rows needs R >= 1 and K a positive multiple of 16 (R=%d, K=%d)", R, K);
    if (nd_misaligned(src_packed, 15) || nd_misaligned(dst, 15)) return nd_set_err(ND_ERR_ARG, "unpack_rows: misaligned tensor (16 bytes)");
    nd_launch_unpack(src_packed, dst, R, K, 0, (hipStream_t)stream);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}
