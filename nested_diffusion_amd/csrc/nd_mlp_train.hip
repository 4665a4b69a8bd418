// nd_mlp_train.hip -- training of the mapping MLPs (include/nested_diffusion.h: nd_linear_wgrad_adam, nd_bias_grad_adam;
// the loop: nested_diffusion_amd/train_mapping.py MappingTrainer).  gfx950 only, all arithmetic fp32.
//   k_wgrad_adam       G[N, K] = gscale * (dy[M, N]^T . x[M, K]) formed 16 x 16 tile by tile on the matrix pipe and applied to the packed
//                      weight, first-moment and second-moment images in registers (torch 1.10 F.adam): the gradient never goes to memory
//   k_bias_grad_adam   the same update for a bias: g[n] = gscale * sum_m dy[m, n]
//   (nd_unpack_rows, the inverse of the images' packing: csrc/nd_pack.hip)
//
// k_wgrad_adam.  v_mfma_f32_16x16x4_f32 computes D[i][j] = sum_kk A[i][kk] B[kk][j] with lane l supplying A[i = l & 15][kk = l >> 4] and
// B[kk = l >> 4][j = l & 15] and receiving D[i = 4 (l >> 4) + e][j = l & 15] in register e.  With A = x^T (lane l: x[4 s + (l >> 4)][k0 +
// (l & 15)]) and B = dy (lane l: dy[4 s + (l >> 4)][n0 + (l & 15)]), summed over the steps s = 0 .. ceil(M / 4) - 1, register e of lane l is
// G[n0 + (l & 15)][k0 + 4 (l >> 4) + e]: the float4 this lane reads from the frag16 block (n0 / 16, k0 / 16) of W, m and v.  The update
// is lane-local: no LDS, no shuffles, one 16-byte load and store per lane, image and block.
//
// Work split: a wave owns WG_KBW adjacent 16-column blocks, keeps their x fragments (ceil(M / 4) registers per block) for its whole life
// and walks a range of row blocks; per row block it loads one dy fragment (from L2: dy is M x N floats) and updates WG_KBW contiguous
// KiB of each image.  The four waves of a workgroup sit side by side (grid.x over K), grid.y splits the row blocks so that small layers
// still fill the chip; x is read once per row-block range.  Every 16 x 16 block is read and written by exactly one wave, once, and its
// result does not depend on the split: the update is race-free in place and has the same bits on every run and under any plan.
// Rows m >= M of the last step and image rows n >= N (the zero padding of nd_pack_rows) get zero operands in registers, never read; the
// gradient of a padding row is forced to 0 after the MFMA and its lanes skip the update, so neither a NaN in x nor eps = 0 reaches the
// padding: it stays exactly 0.
#include "nd_math.hpp"
#include "nd_host.hpp"
#include "nd_optim.hpp"

// every operation of the update (nd_optim.hpp) and of the sums is one rounded fp32 op in the listed order: a float32 restatement on the
// host reproduces it bit for bit on every input, the edges of fp32 included (tests/test_gpu_mlp_edges.py)
#pragma clang fp contract(off)

namespace {

constexpr int WG_WAVES = 4;        // waves per workgroup
constexpr int WG_KBW = 4;          // adjacent 16-column blocks per wave: 4 KiB contiguous per image and row block
constexpr int WG_TARGET = 1024;    // workgroups a launch aims for (grid.y splits the row blocks until grid.x * grid.y reaches it)

struct WgPlan { int gx, gy, rbs; };   // grid and row blocks per workgroup: a function of (N, K) alone
WgPlan wg_plan(int N, int K) {
    const int nkb = K / 16, nrb = (N + 15) / 16, per_wg = WG_WAVES * WG_KBW;
    const int gx = (nkb + per_wg - 1) / per_wg;
    int want = (WG_TARGET + gx - 1) / gx;
    if (want > nrb) want = nrb;
    const int rbs = (nrb + want - 1) / want;
    return WgPlan{gx, (nrb + rbs - 1) / rbs, rbs};
}

template <int MS, bool ADAM>
__global__ __launch_bounds__(WG_WAVES * 64) void k_wgrad_adam(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ w,
                                                             float* __restrict__ mom, float* __restrict__ var, float* __restrict__ g_out, int M,
                                                             int N, int K, int rbs, float gscale, nd_adam_step a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nkb = K >> 4, nrb = (N + 15) >> 4;
    const int kb0 = ((int)blockIdx.x * WG_WAVES + wave) * WG_KBW;
    if (kb0 >= nkb) return;                          // a whole wave past the last column block (no workgroup barrier below)
    const int nb = nkb - kb0 < WG_KBW ? nkb - kb0 : WG_KBW;
    const int q = lane >> 4, c = lane & 15;
    const int rb_lo = (int)blockIdx.y * rbs, rb_hi = rb_lo + rbs < nrb ? rb_lo + rbs : nrb;

    // the x fragments of this wave's column blocks, kept for every row block: xa[i][s] = x[4 s + q][(kb0 + i) * 16 + c], 0 past M.
    // Slots past the image's last column block (i >= nb) repeat the last one; nothing is stored from them.
    float xa[WG_KBW][MS];
#pragma unroll
    for (int i = 0; i < WG_KBW; ++i) {
        const int kb = kb0 + (i < nb ? i : nb - 1);
#pragma unroll
        for (int s = 0; s < MS; ++s) {
            const int mr = 4 * s + q;
            xa[i][s] = mr < M ? x[(size_t)mr * K + (size_t)kb * 16 + c] : 0.f;
        }
    }

    for (int rb = rb_lo; rb < rb_hi; ++rb) {
        const int n = rb * 16 + c;
        const bool live = n < N;
        float d[MS];
#pragma unroll
        for (int s = 0; s < MS; ++s) {
            const int mr = 4 * s + q;
            d[s] = (live && mr < M) ? dy[(size_t)mr * N + n] : 0.f;
        }
        // the images' float4s of all WG_KBW blocks are requested before the first is used (slots i >= nb re-read block nb - 1)
        float4 w4[WG_KBW], m4[WG_KBW], v4[WG_KBW];
        size_t off[WG_KBW];
#pragma unroll
        for (int i = 0; i < WG_KBW; ++i) {
            off[i] = ((size_t)rb * nkb + kb0 + (i < nb ? i : nb - 1)) * 256 + (size_t)lane * 4;
            if (ADAM) {
                w4[i] = *reinterpret_cast<const float4*>(w + off[i]);
                m4[i] = *reinterpret_cast<const float4*>(mom + off[i]);
                v4[i] = *reinterpret_cast<const float4*>(var + off[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < WG_KBW; ++i) {
            f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < MS; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[i][s], d[s], acc, 0, 0, 0);
            // acc[e] = sum_m dy[m][n] x[m][(kb0 + i) * 16 + 4 q + e]
            float4 g;
            g.x = live ? acc[0] * gscale : 0.f;
            g.y = live ? acc[1] * gscale : 0.f;
            g.z = live ? acc[2] * gscale : 0.f;
            g.w = live ? acc[3] * gscale : 0.f;
            if (i < nb) {
                if (g_out) *reinterpret_cast<float4*>(g_out + off[i]) = g;
                if (ADAM && live) {                       // a padding row is not updated at all: it stays 0 whatever eps is (0 / (0 + 0) would be NaN)
                    nd_optim_update(w4[i].x, m4[i].x, v4[i].x, g.x, a);
                    nd_optim_update(w4[i].y, m4[i].y, v4[i].y, g.y, a);
                    nd_optim_update(w4[i].z, m4[i].z, v4[i].z, g.z, a);
                    nd_optim_update(w4[i].w, m4[i].w, v4[i].w, g.w, a);
                }
                if (ADAM) {                               // (the whole wave stores: the padding lanes write back what they read)
                    *reinterpret_cast<float4*>(w + off[i]) = w4[i];
                    *reinterpret_cast<float4*>(mom + off[i]) = m4[i];
                    *reinterpret_cast<float4*>(var + off[i]) = v4[i];
                }
            }
        }
    }
}

template <int MS>
void wg_launch(bool adam, dim3 grid, hipStream_t st, const float* dy, const float* x, float* w, float* m, float* v, float* g, int M, int N, int K,
               int rbs, float gscale, nd_adam_step a) {
    if (adam) hipLaunchKernelGGL((k_wgrad_adam<MS, true>), grid, dim3(WG_WAVES * 64), 0, st, dy, x, w, m, v, g, M, N, K, rbs, gscale, a);
    else hipLaunchKernelGGL((k_wgrad_adam<MS, false>), grid, dim3(WG_WAVES * 64), 0, st, dy, x, w, m, v, g, M, N, K, rbs, gscale, a);
}

// one thread per bias element; the column sum runs m = 0 .. M - 1 in order
__global__ __launch_bounds__(256) void k_bias_grad_adam(const float* __restrict__ dy, float* __restrict__ b, float* __restrict__ mom,
                                                        float* __restrict__ var, float* __restrict__ g_out, int M, int N, float gscale,
                                                        nd_adam_step a, int adam) {
    const int n = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (n >= N) return;
    float acc = 0.f;
    for (int m = 0; m < M; ++m) acc += dy[(size_t)m * N + n];
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

}  // namespace

extern "C" int nd_linear_wgrad_plan(int N, int K, int* out) {
    if (!out) return nd_set_err(ND_ERR_ARG, "linear_wgrad_plan: NULL out");
    if (N < 1 || K < 16 || K % 16) return nd_set_err(ND_ERR_ARG, "linear_wgrad_plan needs N >= 1 and K a positive multiple of 16 (N=%d, K=%d)", N, K);
    const WgPlan p = wg_plan(N, K);
    out[0] = WG_WAVES * WG_KBW;
    out[1] = p.gx;
    out[2] = p.gy;
    out[3] = p.rbs;
    return ND_OK;
}

extern "C" int nd_linear_wgrad_adam(const float* dy, const float* x, void* w_packed, void* m_packed, void* v_packed, void* g_out_packed, int M,
                                    int N, int K, int dtype, float gscale, const nd_adam_step* a, void* stream) {
    if (!dy) return nd_set_err(ND_ERR_ARG, "linear_wgrad_adam: NULL tensor dy");
    if (!x) return nd_set_err(ND_ERR_ARG, "linear_wgrad_adam: NULL tensor x");
    if (!a && !g_out_packed) return nd_set_err(ND_ERR_ARG, "linear_wgrad_adam: both a and g_out are NULL: nothing to write");
    if (a && !w_packed) return nd_set_err(ND_ERR_ARG, "linear_wgrad_adam: NULL image w_packed");
    if (a && !m_packed) return nd_set_err(ND_ERR_ARG, "linear_wgrad_adam: NULL image m_packed");
    if (a && !v_packed) return nd_set_err(ND_ERR_ARG, "linear_wgrad_adam: NULL image v_packed");
    if (dtype != ND_DTYPE_F32)
        return nd_set_err(ND_ERR_ARG, "linear_wgrad_adam: dtype must be ND_DTYPE_F32: the update runs on fp32 (frag16) images only, not on an fp16 image");
    if (M < 1 || M > ND_LINEAR_BWD_MAX_M) return nd_set_err(ND_ERR_ARG, "linear_wgrad_adam needs 1 <= M <= %d (M=%d)", ND_LINEAR_BWD_MAX_M, M);
    if (K < 16 || K % 16) return nd_set_err(ND_ERR_ARG, "linear_wgrad_adam needs K a positive multiple of 16 (K=%d)", K);
    if (N < 1) return nd_set_err(ND_ERR_ARG, "linear_wgrad_adam needs N >= 1 (N=%d)", N);
    if (nd_misaligned(dy, 3) || nd_misaligned(x, 3) || nd_misaligned(w_packed, 15) || nd_misaligned(m_packed, 15) || nd_misaligned(v_packed, 15) ||
        nd_misaligned(g_out_packed, 15))
        return nd_set_err(ND_ERR_ARG, "linear_wgrad_adam: misaligned tensor (the images 16 bytes, dy / x 4)");
    if (a) {
        const void* p[4] = {w_packed, m_packed, v_packed, g_out_packed};
        if (nd_any_equal(p, 4)) return nd_set_err(ND_ERR_ARG, "linear_wgrad_adam: the images w, m, v and g_out must be distinct buffers");
    }
    const WgPlan p = wg_plan(N, K);
    const dim3 grid((unsigned)p.gx, (unsigned)p.gy);
    hipStream_t st = (hipStream_t)stream;
    const nd_adam_step av = a ? *a : nd_adam_step{};
    float *w = (float*)w_packed, *m = (float*)m_packed, *v = (float*)v_packed, *g = (float*)g_out_packed;
    const int steps = (M + 3) / 4;
    if (steps <= 8) wg_launch<8>(a != nullptr, grid, st, dy, x, w, m, v, g, M, N, K, p.rbs, gscale, av);
    else if (steps <= 16) wg_launch<16>(a != nullptr, grid, st, dy, x, w, m, v, g, M, N, K, p.rbs, gscale, av);
    else wg_launch<32>(a != nullptr, grid, st, dy, x, w, m, v, g, M, N, K, p.rbs, gscale, av);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_bias_grad_adam(const float* dy, float* b, float* m, float* v, float* g_out, int M, int N, float gscale, const nd_adam_step* a,
                                 void* stream) {
    if (!dy) return nd_set_err(ND_ERR_ARG, "bias_grad_adam: NULL tensor dy");
    if (!a && !g_out) return nd_set_err(ND_ERR_ARG, "bias_grad_adam: both a and g_out are NULL: nothing to write");
    if (a && !b) return nd_set_err(ND_ERR_ARG, "bias_grad_adam: NULL tensor b");
    if (a && !m) return nd_set_err(ND_ERR_ARG, "bias_grad_adam: NULL tensor m");
    if (a && !v) return nd_set_err(ND_ERR_ARG, "bias_grad_adam: NULL tensor v");
    if (M < 1) return nd_set_err(ND_ERR_ARG, "bias_grad_adam needs M >= 1 (M=%d)", M);
    if (N < 1) return nd_set_err(ND_ERR_ARG, "bias_grad_adam needs N >= 1 (N=%d)", N);
    if (nd_misaligned(dy, 3) || nd_misaligned(b, 3) || nd_misaligned(m, 3) || nd_misaligned(v, 3) || nd_misaligned(g_out, 3))
        return nd_set_err(ND_ERR_ARG, "bias_grad_adam: misaligned tensor");
    if (a) {
        const void* p[4] = {b, m, v, g_out};
        if (nd_any_equal(p, 4)) return nd_set_err(ND_ERR_ARG, "bias_grad_adam: b, m, v and g_out must be distinct buffers");
    }
    const nd_adam_step av = a ? *a : nd_adam_step{};
    hipLaunchKernelGGL(k_bias_grad_adam, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dy, b, m, v, g_out, M, N, gscale, av,
                       a ? 1 : 0);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}
