// nd_gemm_nt.hip -- the large-M GEMM of the ViT (nd_gemm_bias_act; timm 0.4.12 vit_base_patch16_224 semantics, call sites
// classification_train_separately.py:337-340): entry point, tile plan, k-split fixup and the fp16-operand kernel k_gemm_h.  gfx950 only.
// The fp32 kernel k_gemm_nt<128,64> is a unit of its own (nd_gemm_f32.hip: accumulators in VGPRs) behind nd_launch_gemm_nt_128x64.
#include "nd_tile.hpp"
#include "nd_device.hpp"
#include "nd_host.hpp"
#include "nd_vit.hpp"

// ---------------------------------------------------------------------------------------------
// Large-M GEMM, both operands K-contiguous:  out[m,n] = act(sum_k x[m,k] w[n,k] + bias[n]) + res[m,n]
// fp16-operand form (the fp16 mode, BASELINE config 5; not a mode of the reference):
// x stays fp32 in HBM and is rounded to fp16 on its way into LDS, w is an fp16 [N][K] copy made once at load; products are
// exact, accumulation / bias / activation / residual fp32, out fp32.  BK = 32 per stage = one v_mfma_f32_16x16x32_f16 per
// fragment pair; LDS rows are 32 halfs + 8 pad (80 B: the 16 rows of a fragment start at banks 20r mod 64, all distinct,
// so a lane's 8 halfs k = 8*(l>>4)..+7 are one conflict-free ds_read_b128).  Same tile order, tail split and fixup.
// ---------------------------------------------------------------------------------------------
template <int BM, int BN>
__global__ __launch_bounds__(256) void k_gemm_h(const float* __restrict__ x, const _Float16* __restrict__ w,
                                                const float* __restrict__ bias, const float* __restrict__ res,
                                                float* __restrict__ out, int M, int K, int N, int act, int n_full, int split,
                                                float* __restrict__ part) {
    constexpr int WM = BM / 2, WN = BN / 2, FM = WM / 16, FN = WN / 16;
    constexpr int LA = BM * GH_K / 4 / 256;      // float4 (4 fp32) loads per thread for the x tile
    constexpr int LB = BN * GH_K / 8 / 256;      // 16-byte (8 halfs) loads per thread for the w tile
    static_assert(LA >= 1 && LB >= 1, "tile too small");
    __shared__ __attribute__((aligned(16))) _Float16 sA[2][BM][GH_LD];
    __shared__ __attribute__((aligned(16))) _Float16 sB[2][BN][GH_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int tiles_n = (N + BN - 1) / BN;
    const NdTile tl = nd_tile_decode(blockIdx.x, n_full, split);
    const int tm = tl.tile / tiles_n, tn = tl.tile % tiles_n;
    const int m0 = tm * BM, n0 = tn * BN;
    f32x4 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float4 ra[LA];
    f16x8 rb[LB];
#define GH_GLOAD(k0)                                                                                      \
    {                                                                                                     \
        _Pragma("unroll") for (int i = 0; i < LA; ++i) {                                                  \
            const int e = tid + i * 256, row = e >> 3, kq = (e & 7) * 4;                                  \
            ra[i] = *reinterpret_cast<const float4*>(x + (size_t)min(m0 + row, M - 1) * K + (k0) + kq);  \
        }                                                                                                 \
        _Pragma("unroll") for (int i = 0; i < LB; ++i) {                                                  \
            const int e = tid + i * 256, row = e >> 2, kq = (e & 3) * 8;                                  \
            rb[i] = *reinterpret_cast<const f16x8*>(w + (size_t)min(n0 + row, N - 1) * K + (k0) + kq);   \
        }                                                                                                 \
    }
#define GH_SWRITE(buf)                                                                                    \
    {                                                                                                     \
        _Pragma("unroll") for (int i = 0; i < LA; ++i) {                                                  \
            const int e = tid + i * 256, row = e >> 3, kq = (e & 7) * 4;                                  \
            *reinterpret_cast<f16x4*>(&sA[buf][row][kq]) =                                                \
                f16x4{(_Float16)ra[i].x, (_Float16)ra[i].y, (_Float16)ra[i].z, (_Float16)ra[i].w};        \
        }                                                                                                 \
        _Pragma("unroll") for (int i = 0; i < LB; ++i) {                                                  \
            const int e = tid + i * 256, row = e >> 2, kq = (e & 3) * 8;                                  \
            *reinterpret_cast<f16x8*>(&sB[buf][row][kq]) = rb[i];                                         \
        }                                                                                                 \
    }
    const int ks0 = nd_slab_begin(tl.slab, K / GH_K, split), nk = nd_slab_end(tl.slab, K / GH_K, split);
    GH_GLOAD(ks0 * GH_K)
    GH_SWRITE(ks0 & 1)
    __syncthreads();
    const int lr = lane & 15, lk = 8 * (lane >> 4);
    for (int ks = ks0; ks < nk; ++ks) {
        const int buf = ks & 1;
        GH_GLOAD(min(ks + 1, nk - 1) * GH_K)
        f16x8 fa[FM], fb[FN];
#pragma unroll
        for (int i = 0; i < FM; ++i) fa[i] = *reinterpret_cast<const f16x8*>(&sA[buf][wr * WM + 16 * i + lr][lk]);
#pragma unroll
        for (int j = 0; j < FN; ++j) fb[j] = *reinterpret_cast<const f16x8*>(&sB[buf][wc * WN + 16 * j + lr][lk]);
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int j = 0; j < FN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb[j], fa[i], acc[i][j], 0, 0, 0);   // D[i=n][j=m]
        GH_SWRITE(buf ^ 1)
        __syncthreads();
    }
#undef GH_GLOAD
#undef GH_SWRITE
    if (tl.slab >= 0) {
        nd_gemm_store_partial(part + ((size_t)tl.rem_index * split + tl.slab) * (BM * BN), acc, wr * WM + (lane & 15), wc * WN + 4 * (lane >> 4));
        return;
    }
#pragma unroll
    for (int i = 0; i < FM; ++i) {
        const int m = m0 + wr * WM + 16 * i + (lane & 15);
#pragma unroll
        for (int j = 0; j < FN; ++j) {
            const int n = n0 + wc * WN + 16 * j + 4 * (lane >> 4);
            if (m < M && n < N) nd_gemm_finish4(acc[i][j], bias, res, out, act, m, n, N);
        }
    }
}

// Finishes the k-split tiles: out = act(sum_slabs part + bias) + res, slabs added in order (reproducible).
template <int BM, int BN>
__global__ __launch_bounds__(256) void k_gemm_fixup(const float* __restrict__ part, const float* __restrict__ bias,
                                                    const float* __restrict__ res, float* __restrict__ out, int M, int N, int act,
                                                    int n_full, int split) {
    const int tiles_n = (N + BN - 1) / BN;
    const int tile = n_full + blockIdx.y;
    const int m0 = (tile / tiles_n) * BM, n0 = (tile % tiles_n) * BN;
    const int e = blockIdx.x * 256 + threadIdx.x;           // float4 index inside the tile
    const int ml = e / (BN / 4), nl = (e % (BN / 4)) * 4;
    const int m = m0 + ml, n = n0 + nl;
    if (m >= M || n >= N) return;
    const float* pt = part + (size_t)blockIdx.y * split * (BM * BN) + (size_t)ml * BN + nl;
    float4 s4 = *reinterpret_cast<const float4*>(pt);
    for (int k = 1; k < split; ++k) {
        const float4 v = *reinterpret_cast<const float4*>(pt + (size_t)k * (BM * BN));
        s4.x += v.x; s4.y += v.y; s4.z += v.z; s4.w += v.w;
    }
    nd_gemm_finish4(f32x4{s4.x, s4.y, s4.z, s4.w}, bias, res, out, act, m, n, N);
}

// Launch plan.  Measured (tools/bench_gemm2.py): the run time of a launch is ceil(tiles / 256) x (time of one tile), i.e. it
// is quantised on whole tiles per CU, and the 128x64 tile is as fast as 128x128 per flop.  So: 128x64 tiles; the
// tiles % 256 remainder is cut into `split` k-slabs where that shortens the last round (needs the workspace).
#define GT_BM 128
#define GT_BN 64
#define GT_CUS (nd_num_cus())
struct GemmPlan { int tiles, n_full, rem, split; size_t ws_bytes; };
static GemmPlan nd_gemm_plan(int M, int K, int N, int bk = GB_K) {
    GemmPlan p{};
    p.tiles = ((M + GT_BM - 1) / GT_BM) * ((N + GT_BN - 1) / GT_BN);
    const int ncu = GT_CUS;
    p.n_full = (p.tiles / ncu) * ncu;
    p.rem = p.tiles - p.n_full;
    p.split = 1;
    const int nk = K / bk;
    if (p.rem > 0 && (size_t)M * N * K >= ((size_t)1 << 28)) {
        // tail length in tile-times: ceil(rem * s / 256) / s ; take the smallest s that gets within 10 % of the best
        double best = 1e9;
        const int cand[] = {1, 2, 3, 4, 5, 6, 8};
        for (int s : cand) if (nk / s >= 8) best = fmin(best, (double)((p.rem * s + ncu - 1) / ncu) / s);
        for (int s : cand)
            if (nk / s >= 8 && (double)((p.rem * s + ncu - 1) / ncu) / s <= best * 1.1 + 1e-9) { p.split = s; break; }
    }
    p.ws_bytes = p.split > 1 ? (size_t)p.rem * p.split * GT_BM * GT_BN * sizeof(float) : 0;
    return p;
}

// the K step of a dtype's kernel: GB_K / GH_K are what nd_kmul (nd_host.hpp) tells the callers
static_assert(GB_K == 16 && GH_K == 32, "nd_kmul names the K steps of k_gemm_nt and k_gemm_h");

extern "C" size_t nd_gemm_workspace_bytes(int M, int K, int N, int dtype) {
    if (nd_bad_dtype(dtype) || M < 1 || N < 1 || K < nd_kmul(dtype) || (K % nd_kmul(dtype))) return 0;
    return nd_gemm_plan(M, K, N, nd_kmul(dtype)).ws_bytes;
}

extern "C" int nd_gemm_bias_act(const float* x, const void* w, const float* bias, const float* res, float* out, int M, int K,
                                int N, int act, int dtype, void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !w || !out) return nd_set_err(ND_ERR_ARG, "NULL tensor");
    if (nd_bad_dtype(dtype)) return nd_set_err(ND_ERR_ARG, "unknown dtype %d", dtype);
    const int half = dtype == ND_DTYPE_F16, km = nd_kmul(dtype);
    if (M < 1 || N < 1 || K < km || (K % km)) return nd_set_err(ND_ERR_ARG, "need M,N >= 1 and K a positive multiple of %d (K=%d)", km, K);
    if (act < 0 || act > 3) return nd_set_err(ND_ERR_ARG, "unknown activation %d", act);
    hipStream_t st = (hipStream_t)stream;
    GemmPlan p = nd_gemm_plan(M, K, N, km);
    if (p.split > 1 && (!workspace || workspace_bytes < p.ws_bytes || ((uintptr_t)workspace & 15))) {
        // no (or too small / misaligned) workspace: every tile whole -- same results up to summation order, longer tail
        p.n_full = p.tiles; p.rem = 0; p.split = 1;
    }
    if (p.split == 1) { p.n_full = p.tiles; p.rem = 0; }
    float* part = (float*)workspace;
    const dim3 grid((unsigned)(p.n_full + p.rem * p.split));
    if (half)
        hipLaunchKernelGGL((k_gemm_h<GT_BM, GT_BN>), grid, dim3(256), 0, st, x, (const _Float16*)w, bias, res, out, M, K, N, act, p.n_full,
                           p.split, part);
    else
        HIP_CHECK(nd_launch_gemm_nt_128x64(x, (const float*)w, bias, res, out, M, K, N, act, p.n_full, p.split, part, grid.x, st));
    HIP_CHECK(hipGetLastError());
    if (p.rem > 0) {
        hipLaunchKernelGGL((k_gemm_fixup<GT_BM, GT_BN>), dim3(GT_BM * GT_BN / 4 / 256, p.rem), dim3(256), 0, st, part, bias, res, out, M, N,
                           act, p.n_full, p.split);
        HIP_CHECK(hipGetLastError());
    }
    return ND_OK;
}
