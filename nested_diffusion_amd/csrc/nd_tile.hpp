// nd_tile.hpp -- what the LDS-tiled kernels share besides their main loops (nd_gemm_f32.hip, nd_gemm_nt.hip, nd_gemm_b9.hip,
// nd_cond_gemm.hip, nd_attention.hip, nd_attention_b9.hip): the order in which a launch's workgroups take its tiles, and the epilogue
// of a lane's four output columns.  The tile order is plain integer arithmetic (host and device: tools/check_tile_order.hip walks it
// on the CPU); the epilogue is device-only inline code.  gfx950 / CDNA4 only.
#pragma once
#include "nd_math.hpp"

// ---- tile order ----------------------------------------------------------------------------------------------------------------------
// Workgroups are dispatched to the 8 XCDs round-robin, so blocks b and b + 8 share an XCD and its L2.  Of `total` work items, XCD x takes
// the contiguous run [x*q + min(x, r), ...) of q + 1 (x < r) or q items (q = total / 8, r = total % 8), in dispatch order: the workgroups
// that share an L2 then work on neighbouring tiles (one x panel of a GEMM; the K / V of one head).
__host__ __device__ __forceinline__ int nd_xcd_run(int bid, int total) {
    const int q = total / 8, r = total % 8, xcd = bid % 8, loc = bid / 8;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
}

// Which tile a workgroup of a (whole tiles + k-split remainder) launch owns.  Workgroups [0, n_full) take one whole tile each (slab -1),
// dealt to the XCDs in runs; the tiles from n_full on -- the last, partly empty round -- are cut into `split` >= 1 k-slabs, one workgroup
// per slab, slabs of a tile adjacent: remainder tile rem_index = tile - n_full, raw sums to a workspace, finished by a fixup launch.
struct NdTile { int tile, slab, rem_index; };
__host__ __device__ __forceinline__ NdTile nd_tile_decode(int bid, int n_full, int split) {
    if (bid < n_full) return NdTile{nd_xcd_run(bid, n_full), -1, 0};
    const int j = bid - n_full, ri = j / split;
    return NdTile{n_full + ri, j % split, ri};
}

// K-steps [begin, end) of a slab out of nk: the `split` slabs of a tile partition [0, nk); slab -1 is the whole range
__host__ __device__ __forceinline__ int nd_slab_begin(int slab, int nk, int split) { return slab < 0 ? 0 : (int)((long)slab * nk / split); }
__host__ __device__ __forceinline__ int nd_slab_end(int slab, int nk, int split) { return slab < 0 ? nk : (int)((long)(slab + 1) * nk / split); }

// ---- epilogue of a lane's four consecutive output columns n .. n+3 of row m (m < M, n < N: the caller's check) ------------------------
// v = act(acc + bias[n]) + res[m,n]; columns past N read clamped bias, no residual, and are never stored
__device__ __forceinline__ void nd_gemm_values4(f32x4 acc, const float* bias, const float* res, int act, int m, int n, int N, float (&v)[4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int nn = min(n + r, N - 1);
        float t = acc[r] + (bias ? bias[nn] : 0.f);
        t = nd_act(t, act);
        if (res && n + r < N) t += res[(size_t)m * N + n + r];
        v[r] = t;
    }
}

// row-major [M][N] store: one 16-byte store where the row keeps it aligned and whole, else the columns below N one by one
__device__ __forceinline__ void nd_store_row4(float* out, int m, int n, int N, const float (&v)[4]) {
    float* p = out + (size_t)m * N + n;
    if (n + 3 < N && (N & 3) == 0) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else {
#pragma unroll
        for (int r = 0; r < 4; ++r) if (n + r < N) p[r] = v[r];
    }
}

__device__ __forceinline__ void nd_gemm_finish4(f32x4 acc, const float* bias, const float* res, float* out, int act, int m, int n, int N) {
    float v[4];
    nd_gemm_values4(acc, bias, res, act, m, n, N, v);
    nd_store_row4(out, m, n, N, v);
}

// raw accumulators of a k-slab into its [BM][BN] fp32 workspace tile (2 x 2 waves of FM x FN fragments: BN = 32 FN); the lane's first
// row ml and column nl inside the tile: it holds D[n = 4*(l>>4) + r][m = l&15], 4 consecutive n of one row m, per fragment
template <int FM, int FN>
__device__ __forceinline__ void nd_gemm_store_partial(float* tile, const f32x4 (&acc)[FM][FN], int ml, int nl) {
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) *reinterpret_cast<f32x4*>(tile + (ml + 16 * i) * (32 * FN) + nl + 16 * j) = acc[i][j];
}
