// nd_vit_train.hip -- training of the ViT (include/nested_diffusion.h: nd_gemm_tn_adamw, nd_gemm_tn_plan, nd_colsum_adamw,
// nd_layernorm_wgrad_adamw; the loop: nested_diffusion_amd/train_transformer.py ViTTrainer).  gfx950 only, all arithmetic fp32.
//   k_gemm_tn_adamw    G[N, K] = gscale * (dy[M, N]^T . x[M, K]) for a contraction of thousands of rows: a workgroup owns one
//                      GT_TN x GT_TK tile of G, walks M in stages of GT_MT rows staged through LDS, and applies torch 1.10's
//                      F.adamw to the ROW-MAJOR fp32 weight, first and second moment in registers: the gradient never goes to memory
//   k_colsum_adamw     the same update for a vector parameter (bias, pos_embed, cls_token): g[n] = gscale * sum_m dy[m, n]
//   k_ln_wgrad_partial / k_ln_wgrad_finish   LayerNorm's gamma / beta: dgamma[c] = sum_r g[r, c] xhat[r, c], dbeta[c] = sum_r g[r, c],
//                      xhat recomputed; per-chunk partials through a caller-owned workspace, then the ordered sum and the update
//
// k_gemm_tn_adamw.  v_mfma_f32_16x16x4_f32 computes D[i][j] = sum_kk A[i][kk] B[kk][j] with lane l supplying A[i = l & 15][kk = l >> 4]
// and B[kk = l >> 4][j = l & 15] and receiving D[i = 4 (l >> 4) + e][j = l & 15] in register e.  With A = dy^T and B = x both operands
// are read in the layout they arrive in: lane l takes dy[m0 + (l >> 4)][n0 + (l & 15)] and x[m0 + (l >> 4)][k0 + (l & 15)] -- 16
// consecutive floats of 4 consecutive rows, from an LDS stage whose row stride (GT_LD = 80 floats, 16 mod 64 banks) spreads the 4
// rows over the 64 banks.  Register e of lane l is G[n0 + 4 (l >> 4) + e][k0 + (l & 15)]: the 16 lanes of a quarter wave store 64
// contiguous bytes of a row of w, m and v.  The accumulator of a 16 x 16 tile is carried through EVERY step of the M loop, so each
// output element is one fma chain over m = 0 .. M - 1 (the instruction itself is a k-ordered fma chain): its bits depend on
// the shape alone, not on the tile the element falls in, the grid, or the run.  Rows past M, columns n >= N and k >= K are zero
// operands written into the stage, never read from memory; their results are never stored.
//
// The next stage's global loads are issued into registers before the MFMAs of the current one (one LDS buffer, two barriers a stage).
//
// Summation order of k_colsum_adamw and k_ln_wgrad_partial / _finish (ND_COLSUM_CHUNK = 64): the rows are cut into chunks of 64 (the last one
// shorter); a chunk's partial is p = 0, p += term(r) for r in row order; the result is acc = 0, acc += p in chunk order.  A function of
// the row count alone: not of the width, the grid or which wave summed a chunk.
#include "nd_math.hpp"
#include "nd_host.hpp"
#include "nd_optim.hpp"

// every operation of the update (nd_optim.hpp) and of the sums is one rounded fp32 op in the listed order: a float32 restatement on the
// host reproduces them bit for bit (tests/test_gpu_vit_train.py)
#pragma clang fp contract(off)

namespace {

constexpr int GT_TN = 64, GT_TK = 64;   // the tile of G a workgroup owns: four waves, a 32 x 32 quadrant (2 x 2 MFMA tiles) each
constexpr int GT_MT = 32;               // rows of dy / x per LDS stage
constexpr int GT_LD = 80;               // LDS row stride in floats
constexpr int GT_PER = GT_MT * 64 / 256;   // elements of each operand a thread stages

constexpr int CS_CHUNK = ND_COLSUM_CHUNK;

template <bool ADAM>
__global__ __launch_bounds__(256) void k_gemm_tn_adamw(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ w,
                                                       float* __restrict__ mom, float* __restrict__ var, float* __restrict__ g_out, int M,
                                                       int N, int K, float gscale, nd_adamw_step a) {
    __shared__ float sa[GT_MT * GT_LD], sb[GT_MT * GT_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = lane >> 4, c = lane & 15;
    const int n0 = (int)blockIdx.y * GT_TN, k0 = (int)blockIdx.x * GT_TK;
    const int wn = (wave >> 1) * 32, wk = (wave & 1) * 32;
    // staging: thread t moves column (t & 63) of rows (t >> 6) + 4 i, i = 0 .. GT_PER - 1, of both operands
    const int sc = tid & 63, sr = tid >> 6;
    const bool a_live = n0 + sc < N, b_live = k0 + sc < K;
    float ra[GT_PER], rb[GT_PER];
#pragma unroll
    for (int i = 0; i < GT_PER; ++i) {
        const int mr = sr + 4 * i;
        ra[i] = (a_live && mr < M) ? dy[(size_t)mr * N + n0 + sc] : 0.f;
        rb[i] = (b_live && mr < M) ? x[(size_t)mr * K + k0 + sc] : 0.f;
    }
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int m0 = 0; m0 < M; m0 += GT_MT) {
#pragma unroll
        for (int i = 0; i < GT_PER; ++i) {
            sa[(sr + 4 * i) * GT_LD + sc] = ra[i];
            sb[(sr + 4 * i) * GT_LD + sc] = rb[i];
        }
        __syncthreads();
        const int m1 = m0 + GT_MT;
        if (m1 < M) {
#pragma unroll
            for (int i = 0; i < GT_PER; ++i) {
                const int mr = m1 + sr + 4 * i;
                ra[i] = (a_live && mr < M) ? dy[(size_t)mr * N + n0 + sc] : 0.f;
                rb[i] = (b_live && mr < M) ? x[(size_t)mr * K + k0 + sc] : 0.f;
            }
        }
        const int left = M - m0, steps = left >= GT_MT ? GT_MT / 4 : (left + 3) / 4;   // the same for the whole workgroup
        for (int s = 0; s < steps; ++s) {
            const int row = (4 * s + q) * GT_LD;
            const float a0 = sa[row + wn + c], a1 = sa[row + wn + 16 + c];
            const float b0 = sb[row + wk + c], b1 = sb[row + wk + 16 + c];
            acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }

    // acc[i][j][e] = sum_m dy[m][n] x[m][k], n = n0 + wn + 16 i + 4 q + e, k = k0 + wk + 16 j + c
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int k = k0 + wk + 16 * j + c;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int n = n0 + wn + 16 * i + 4 * q + e;
                if (n < N && k < K) {
                    const size_t off = (size_t)n * K + k;
                    const float g = acc[i][j][e] * gscale;
                    if (g_out) g_out[off] = g;
                    if (ADAM) {
                        float wv = w[off], mv = mom[off], vv = var[off];
                        nd_optim_update(wv, mv, vv, g, a);
                        w[off] = wv;
                        mom[off] = mv;
                        var[off] = vv;
                    }
                }
            }
        }
}

// COLS columns x GROUPS row groups a workgroup (1024 threads).  Round r: group j sums chunk r * GROUPS + j in row order; then the first
// group adds the round's partials to its accumulator in chunk order.  Few rows: 64 columns x 16 groups (whole 256-byte rows of dy per
// wave); many rows (the biases at thousands of token rows, where N is a few hundred columns): 16 x 64, four times the workgroups and
// the chunks of a round.  The order, and with it the bits, is the same in both.
template <int COLS, int GROUPS>
__global__ __launch_bounds__(COLS * GROUPS) void k_colsum_adamw(const float* __restrict__ dy, float* __restrict__ b, float* __restrict__ mom,
                                                                float* __restrict__ var, float* __restrict__ g_out, int M, int N,
                                                                float gscale, nd_adamw_step a, int adam) {
    __shared__ float part[GROUPS][COLS];
    const int col = threadIdx.x % COLS, grp = threadIdx.x / COLS;
    const long n = (long)blockIdx.x * COLS + col;
    const bool live = n < N;
    const int nchunks = (M + CS_CHUNK - 1) / CS_CHUNK;
    float acc = 0.f;
    for (int c0 = 0; c0 < nchunks; c0 += GROUPS) {         // uniform over the workgroup: the barriers are met by every thread
        const int ch = c0 + grp;
        float p = 0.f;
        if (live && ch < nchunks) {
            const int r0 = ch * CS_CHUNK, r1 = r0 + CS_CHUNK < M ? r0 + CS_CHUNK : M;
            for (int r = r0; r < r1; ++r) p += dy[(size_t)r * N + n];
        }
        part[grp][col] = p;
        __syncthreads();
        if (grp == 0) {
            const int cnt = nchunks - c0 < GROUPS ? nchunks - c0 : GROUPS;
            for (int j = 0; j < cnt; ++j) acc += part[j][col];
        }
        __syncthreads();
    }
    if (grp != 0 || !live) return;
    const float g = acc * gscale;
    if (g_out) g_out[n] = g;
    if (adam) {
        float wv = b[n], mv = mom[n], vv = var[n];
        nd_optim_update(wv, mv, vv, g, a);
        b[n] = wv;
        mom[n] = mv;
        var[n] = vv;
    }
}

// Two launches over a caller-owned workspace of one partial per chunk.  k_ln_wgrad_partial: one wave per chunk (and per workgroup: the
// chunks spread over the CUs).  The wave holds whole rows (VPL float4 per lane and row, the layout of k_layernorm / k_layernorm_bwd), so
// the statistics are nd_ln_stats' and xhat = ((x - mean) - cm) * rstd is k_layernorm_bwd's; R rows are loaded ahead of their reductions
// and added in row order.  It writes part[chunk][0][c] = sum g xhat, part[chunk][1][c] = sum g.  k_ln_wgrad_finish: one thread per
// column adds the partials in chunk order and applies the update.
template <int VPL, int R>
__global__ __launch_bounds__(64) void k_ln_wgrad_partial(const float* __restrict__ x, const float* __restrict__ g, float* __restrict__ part, int rows,
                                                        int dim, float eps) {
    static_assert(CS_CHUNK % R == 0, "a chunk is a whole number of row groups");
    const int lane = threadIdx.x, ch = blockIdx.x;
    const int r0 = ch * CS_CHUNK, r1 = r0 + CS_CHUNK < rows ? r0 + CS_CHUNK : rows;
    float4 pg[VPL], pb[VPL];
#pragma unroll
    for (int i = 0; i < VPL; ++i) pg[i] = pb[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int r = r0; r < r1; r += R) {
        float4 v[R][VPL], gv[R][VPL];
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const bool in = r + j < r1;                        // rows past the chunk: zeros in registers, never read, never added
            const size_t base = (size_t)(r + j) * dim;
#pragma unroll
            for (int i = 0; i < VPL; ++i) {
                const int c = (i * 64 + lane) * 4;
                const bool ld = in && c < dim;
                v[j][i] = ld ? *reinterpret_cast<const float4*>(x + base + c) : make_float4(0.f, 0.f, 0.f, 0.f);
                gv[j][i] = ld ? *reinterpret_cast<const float4*>(g + base + c) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        float mean[R], cm[R], rstd[R];
#pragma unroll
        for (int j = 0; j < R; ++j) nd_ln_stats<VPL>(v[j], lane, dim, eps, mean[j], cm[j], rstd[j]);
#pragma unroll
        for (int j = 0; j < R; ++j) {
            if (r + j < r1) {
#pragma unroll
                for (int i = 0; i < VPL; ++i) {
                    if ((i * 64 + lane) * 4 < dim) {
                        pg[i].x += gv[j][i].x * (((v[j][i].x - mean[j]) - cm[j]) * rstd[j]);
                        pg[i].y += gv[j][i].y * (((v[j][i].y - mean[j]) - cm[j]) * rstd[j]);
                        pg[i].z += gv[j][i].z * (((v[j][i].z - mean[j]) - cm[j]) * rstd[j]);
                        pg[i].w += gv[j][i].w * (((v[j][i].w - mean[j]) - cm[j]) * rstd[j]);
                        pb[i].x += gv[j][i].x;
                        pb[i].y += gv[j][i].y;
                        pb[i].z += gv[j][i].z;
                        pb[i].w += gv[j][i].w;
                    }
                }
            }
        }
    }
    float* out = part + (size_t)ch * 2 * dim;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (c < dim) {
            *reinterpret_cast<float4*>(out + c) = pg[i];
            *reinterpret_cast<float4*>(out + dim + c) = pb[i];
        }
    }
}

__global__ __launch_bounds__(64) void k_ln_wgrad_finish(const float* __restrict__ part, float* __restrict__ gamma, float* __restrict__ beta,
                                                       float* __restrict__ m_gamma, float* __restrict__ v_gamma, float* __restrict__ m_beta,
                                                       float* __restrict__ v_beta, float* __restrict__ go_gamma, float* __restrict__ go_beta,
                                                       int nchunks, int dim, float gscale, nd_adamw_step a, int adam) {
    const int c = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (c >= dim) return;
    float sg = 0.f, sb = 0.f;
    for (int ch = 0; ch < nchunks; ++ch) {
        sg += part[(size_t)ch * 2 * dim + c];
        sb += part[(size_t)ch * 2 * dim + dim + c];
    }
    const float dg = sg * gscale, db = sb * gscale;
    if (go_gamma) go_gamma[c] = dg;
    if (go_beta) go_beta[c] = db;
    if (adam) {
        float wv = gamma[c], mv = m_gamma[c], vv = v_gamma[c];
        nd_optim_update(wv, mv, vv, dg, a);
        gamma[c] = wv;
        m_gamma[c] = mv;
        v_gamma[c] = vv;
        wv = beta[c], mv = m_beta[c], vv = v_beta[c];
        nd_optim_update(wv, mv, vv, db, a);
        beta[c] = wv;
        m_beta[c] = mv;
        v_beta[c] = vv;
    }
}

bool ln_shape_ok(int rows, int dim) { return rows >= 1 && dim >= 4 && dim % 4 == 0 && dim <= 2048; }

}  // namespace

extern "C" int nd_gemm_tn_plan(int N, int K, int* out) {
    if (!out) return nd_set_err(ND_ERR_ARG, "gemm_tn_plan: NULL out");
    if (N < 1 || K < 16 || K % 16) return nd_set_err(ND_ERR_ARG, "gemm_tn_plan needs N >= 1 and K a positive multiple of 16 (N=%d, K=%d)", N, K);
    out[0] = GT_TN;
    out[1] = GT_TK;
    out[2] = GT_MT;
    out[3] = (K + GT_TK - 1) / GT_TK;
    out[4] = (N + GT_TN - 1) / GT_TN;
    return ND_OK;
}

extern "C" int nd_gemm_tn_adamw(const float* dy, const float* x, float* w, float* m, float* v, float* g_out, int M, int N, int K, float gscale,
                                const nd_adamw_step* a, void* stream) {
    if (!dy) return nd_set_err(ND_ERR_ARG, "gemm_tn_adamw: NULL tensor dy");
    if (!x) return nd_set_err(ND_ERR_ARG, "gemm_tn_adamw: NULL tensor x");
    if (!a && !g_out) return nd_set_err(ND_ERR_ARG, "gemm_tn_adamw: both a and g_out are NULL: nothing to write");
    if (a && !w) return nd_set_err(ND_ERR_ARG, "gemm_tn_adamw: NULL tensor w");
    if (a && !m) return nd_set_err(ND_ERR_ARG, "gemm_tn_adamw: NULL tensor m");
    if (a && !v) return nd_set_err(ND_ERR_ARG, "gemm_tn_adamw: NULL tensor v");
    if (M < 1) return nd_set_err(ND_ERR_ARG, "gemm_tn_adamw needs M >= 1 (M=%d)", M);
    if (N < 1) return nd_set_err(ND_ERR_ARG, "gemm_tn_adamw needs N >= 1 (N=%d)", N);
    if (K < 16 || K % 16) return nd_set_err(ND_ERR_ARG, "gemm_tn_adamw needs K a positive multiple of 16 (K=%d)", K);
    if ((N + GT_TN - 1) / GT_TN > 65535) return nd_set_err(ND_ERR_ARG, "gemm_tn_adamw: N too large (N=%d)", N);
    if (nd_misaligned(dy, 3) || nd_misaligned(x, 3) || nd_misaligned(w, 3) || nd_misaligned(m, 3) || nd_misaligned(v, 3) || nd_misaligned(g_out, 3))
        return nd_set_err(ND_ERR_ARG, "gemm_tn_adamw: misaligned tensor");
    if (a) {
        const void* p[4] = {w, m, v, g_out};
        if (nd_any_equal(p, 4)) return nd_set_err(ND_ERR_ARG, "gemm_tn_adamw: w, m, v and g_out must be distinct buffers");
    }
    const dim3 grid((unsigned)((K + GT_TK - 1) / GT_TK), (unsigned)((N + GT_TN - 1) / GT_TN));
    const nd_adamw_step av = a ? *a : nd_adamw_step{};
    hipStream_t st = (hipStream_t)stream;
    if (a) hipLaunchKernelGGL((k_gemm_tn_adamw<true>), grid, dim3(256), 0, st, dy, x, w, m, v, g_out, M, N, K, gscale, av);
    else hipLaunchKernelGGL((k_gemm_tn_adamw<false>), grid, dim3(256), 0, st, dy, x, w, m, v, g_out, M, N, K, gscale, av);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_colsum_adamw(const float* dy, float* b, float* m, float* v, float* g_out, int M, int N, float gscale, const nd_adamw_step* a,
                               void* stream) {
    if (!dy) return nd_set_err(ND_ERR_ARG, "colsum_adamw: NULL tensor dy");
    if (!a && !g_out) return nd_set_err(ND_ERR_ARG, "colsum_adamw: both a and g_out are NULL: nothing to write");
    if (a && !b) return nd_set_err(ND_ERR_ARG, "colsum_adamw: NULL tensor b");
    if (a && !m) return nd_set_err(ND_ERR_ARG, "colsum_adamw: NULL tensor m");
    if (a && !v) return nd_set_err(ND_ERR_ARG, "colsum_adamw: NULL tensor v");
    if (M < 1) return nd_set_err(ND_ERR_ARG, "colsum_adamw needs M >= 1 (M=%d)", M);
    if (N < 1) return nd_set_err(ND_ERR_ARG, "colsum_adamw needs N >= 1 (N=%d)", N);
    if (nd_misaligned(dy, 3) || nd_misaligned(b, 3) || nd_misaligned(m, 3) || nd_misaligned(v, 3) || nd_misaligned(g_out, 3))
        return nd_set_err(ND_ERR_ARG, "colsum_adamw: misaligned tensor");
    if (a) {
        const void* p[4] = {b, m, v, g_out};
        if (nd_any_equal(p, 4)) return nd_set_err(ND_ERR_ARG, "colsum_adamw: b, m, v and g_out must be distinct buffers");
    }
    const nd_adamw_step av = a ? *a : nd_adamw_step{};
    if (M > 2 * CS_CHUNK)
        hipLaunchKernelGGL((k_colsum_adamw<16, 64>), dim3((unsigned)((N + 15) / 16)), dim3(1024), 0, (hipStream_t)stream, dy, b, m, v, g_out, M, N,
                           gscale, av, a ? 1 : 0);
    else
        hipLaunchKernelGGL((k_colsum_adamw<64, 16>), dim3((unsigned)((N + 63) / 64)), dim3(1024), 0, (hipStream_t)stream, dy, b, m, v, g_out, M, N,
                           gscale, av, a ? 1 : 0);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" size_t nd_layernorm_wgrad_workspace_bytes(int rows, int dim) {
    if (!ln_shape_ok(rows, dim)) return 0;
    return (size_t)((rows + CS_CHUNK - 1) / CS_CHUNK) * 2 * (size_t)dim * sizeof(float);
}

extern "C" int nd_layernorm_wgrad_adamw(const float* x, const float* g, float* gamma, float* beta, float* m_gamma, float* v_gamma, float* m_beta,
                                        float* v_beta, float* g_out_gamma, float* g_out_beta, int rows, int dim, float eps, float gscale,
                                        const nd_adamw_step* a, void* ws, size_t ws_bytes, void* stream) {
    if (!x) return nd_set_err(ND_ERR_ARG, "layernorm_wgrad_adamw: NULL tensor x");
    if (!g) return nd_set_err(ND_ERR_ARG, "layernorm_wgrad_adamw: NULL tensor g");
    if (!a && !g_out_gamma && !g_out_beta) return nd_set_err(ND_ERR_ARG, "layernorm_wgrad_adamw: a and both g_out are NULL: nothing to write");
    if (a && (!gamma || !beta || !m_gamma || !v_gamma || !m_beta || !v_beta))
        return nd_set_err(ND_ERR_ARG, "layernorm_wgrad_adamw: NULL parameter or moment tensor");
    if (!ln_shape_ok(rows, dim))
        return nd_set_err(ND_ERR_ARG, "layernorm_wgrad_adamw needs rows >= 1, dim %% 4 == 0, 4 <= dim <= 2048 (rows=%d, dim=%d)", rows, dim);
    const size_t need = nd_layernorm_wgrad_workspace_bytes(rows, dim);
    if (!ws || ws_bytes < need)
        return nd_set_err(ND_ERR_ARG, "layernorm_wgrad_adamw: workspace of %zu bytes, %zu needed (nd_layernorm_wgrad_workspace_bytes)", ws ? ws_bytes : (size_t)0, need);
    if (nd_misaligned(x, 15) || nd_misaligned(g, 15) || nd_misaligned(ws, 15) || nd_misaligned(gamma, 3) || nd_misaligned(beta, 3) || nd_misaligned(m_gamma, 3) ||
        nd_misaligned(v_gamma, 3) || nd_misaligned(m_beta, 3) || nd_misaligned(v_beta, 3) || nd_misaligned(g_out_gamma, 3) || nd_misaligned(g_out_beta, 3))
        return nd_set_err(ND_ERR_ARG, "layernorm_wgrad_adamw: misaligned tensor (x / g / workspace 16 bytes, the rest 4)");
    if (a) {
        const void* p[8] = {gamma, beta, m_gamma, v_gamma, m_beta, v_beta, g_out_gamma, g_out_beta};
        if (nd_any_equal(p, 8)) return nd_set_err(ND_ERR_ARG, "layernorm_wgrad_adamw: the parameter, moment and g_out tensors must be distinct buffers");
    }
    const nd_adamw_step av = a ? *a : nd_adamw_step{};
    hipStream_t st = (hipStream_t)stream;
    const int vpl = (dim / 4 + 63) / 64, nchunks = (rows + CS_CHUNK - 1) / CS_CHUNK;
    float* part = (float*)ws;
#define ND_LW_LAUNCH(V, R) hipLaunchKernelGGL((k_ln_wgrad_partial<V, R>), dim3((unsigned)nchunks), dim3(64), 0, st, x, g, part, rows, dim, eps)
    if (vpl <= 1) ND_LW_LAUNCH(1, 4);
    else if (vpl <= 2) ND_LW_LAUNCH(2, 4);
    else if (vpl <= 3) ND_LW_LAUNCH(3, 4);
    else if (vpl <= 4) ND_LW_LAUNCH(4, 2);
    else ND_LW_LAUNCH(8, 2);
#undef ND_LW_LAUNCH
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_ln_wgrad_finish, dim3((unsigned)((dim + 63) / 64)), dim3(64), 0, st, part, gamma, beta, m_gamma, v_gamma, m_beta, v_beta,
                       g_out_gamma, g_out_beta, nchunks, dim, gscale, av, a ? 1 : 0);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}
