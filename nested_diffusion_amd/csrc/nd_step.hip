// nd_step.hip -- the per-step kernels of the DDPM reverse loop in its hipGraph form: the step head (two layouts) and the last step.
// Arithmetic and argument tables: nd_step.hpp; who launches them: csrc/nd_sampler.hip.  gfx950 only.
//
// Reference path (file:line relative to the reference checkout):
//   diffusion/diffusion_utils.py:54-111    p_sample / p_sample_t_1to0
//   diffusion/latent_model.py:93-105,169-184  ConditionalLinear / ConditionalModel.forward
#include "nd_frag.hpp"
#include "nd_step.hpp"
#include "nd_b9.hpp"

// eps[m, c] = sum over the n-tiles of lin3's projected partials (lin4.bias added by the caller); fixed
// reduction tree (thread-strided, wave shuffle, then waves in order) => reproducible.  All C classes
// are reduced in one pass (C is a template parameter: everything stays in registers).
template <int NT_THREADS, int C>
__device__ __forceinline__ void nd_reduce_eps(const float* __restrict__ epart, int NT, int m, float* red /* [NT_THREADS/64][C] */,
                                              float (&out)[C]) {
    const int tid = threadIdx.x;
    float s[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        s[c] = 0.f;
        nd_gcf row = ND_GC(epart + ((size_t)m * C + c) * NT);
        for (int tl = tid; tl < NT; tl += NT_THREADS) s[c] += row[tl];
    }
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s[c] += __shfl_down(s[c], off, 64);
    if ((tid & 63) == 0)
#pragma unroll
        for (int c = 0; c < C; ++c) red[(tid >> 6) * C + c] = s[c];
    __syncthreads();
#pragma unroll
    for (int c = 0; c < C; ++c) {
        float tot = 0.f;
#pragma unroll
        for (int w = 0; w < NT_THREADS / 64; ++w) tot += red[w * C + c];
        out[c] = tot;
    }
}

// Step head: finish the previous step (reduce eps, posterior update -> y_t), then the first
// ConditionalLinear block of this step:  h1 = softplus(A1[t] * (lin1.W [y_t, yhat]) + C1[t]) * xe
// (latent_model.py:173-177).  Grid (ceil(F/1024), M, members), 256 threads, 4 columns per thread.
// Every thread computes y_t redundantly (C values), so nothing crosses threads after the reduce; the
// table / xe / lin1 loads are issued before the reduction so their latency overlaps it.
// COEF (a sampler plan, nd_set_sampler): the update is nd_coef_update with row t_prev of the plan's table (io.alphas), see nd_step.hpp.
template <int C, bool COEF = false>
__global__ __launch_bounds__(256) void k_step_head(MemberInline mi, const MemberDev* __restrict__ members, StepIO io, int mode, int i_step,
                                                   int t_prev, int t, int B, int M, int maxM, int F, int NT, int T) {
    typedef const __attribute__((address_space(4))) char* nd_cbytes;           // scalar loads from either source (see k_skinny)
    const MemberDev mb = nd_ldc<MemberDev>((members ? (nd_cbytes)(uintptr_t)members : (nd_cbytes)__builtin_amdgcn_kernarg_segment_ptr()) +
                                           (size_t)blockIdx.z * sizeof(MemberDev));
    const int z = blockIdx.z, m = blockIdx.y, b = m % B, tid = threadIdx.x;
    __shared__ float red[4 * C];
    const int n = blockIdx.x * 1024 + tid * 4;
    const bool live = n < F;
    const int nchF = F >> 4;
    constexpr int C2 = 2 * C;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), cc = a, xe = a;
    float w1[4][C2];
    if (live) {
        a = nd_ld16<false>(mb.A1 + (size_t)t * F + n);
        cc = nd_ld16<false>(mb.C1 + (size_t)t * F + n);
        xe = nd_ld16<false>(mb.xe + nd_pk(b, n, nchF));
        nd_gcf wrow = ND_GC(mb.lin1_w + (size_t)n * C2);     // 4 consecutive rows = 4*C2 contiguous floats
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int q = 0; q < C2; ++q) w1[j][q] = wrow[j * C2 + q];
    }
    const int par_new = i_step & 1;                       // ybuf parity written by this step
    nd_gf ynew = ND_GW(mb.ybuf + ((size_t)par_new * maxM + m) * C);
    nd_gcf yold = ND_GC(mb.ybuf + ((size_t)(par_new ^ 1) * maxM + m) * C);
    float yv[C], yh[C], ym[C], zz[C], yo[C], eps[C];
    float al = 0.f, s_t = 0.f, s_tm1 = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        yh[c] = ND_GC(io.yhat)[z * io.yhat_ms + (size_t)b * C + c];
        eps[c] = 0.f; ym[c] = 0.f; zz[c] = 0.f; yo[c] = 0.f;
    }
    if (mode != ND_HEAD_GIVEN) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            ym[c] = ND_GC(io.ymean)[z * io.ymean_ms + (size_t)b * C + c];
            zz[c] = ND_GC(io.noise)[z * io.noise_ms + ((size_t)i_step * M + m) * C + c];
        }
    }
    float cf[4] = {0.f, 0.f, 0.f, 0.f};
    if (mode == ND_HEAD_UPDATE) {
        if constexpr (COEF) {
#pragma unroll
            for (int q = 0; q < 4; ++q) cf[q] = ND_GC(io.alphas)[4 * t_prev + q];
        } else {
            al = ND_GC(io.alphas)[t_prev]; s_t = ND_GC(io.omabs)[t_prev]; s_tm1 = ND_GC(io.omabs)[t_prev - 1];
        }
#pragma unroll
        for (int c = 0; c < C; ++c) yo[c] = yold[c];
        nd_reduce_eps<256, C>(mb.epart, NT, m, red, eps);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        if (mode == ND_HEAD_INIT) yv[c] = zz[c] + ym[c];
        else if (mode == ND_HEAD_UPDATE)
            yv[c] = COEF ? nd_coef_update(yo[c], ym[c], eps[c] + ND_GC(mb.lin4_b)[c], zz[c], cf[0], cf[1], cf[2], cf[3])
                         : nd_posterior(yo[c], ym[c], eps[c] + ND_GC(mb.lin4_b)[c], zz[c], al, s_t, s_tm1);
        else yv[c] = ND_GC(io.y_in)[z * io.yin_ms + (size_t)m * C + c];
        if (tid == 0 && blockIdx.x == 0) {
            ynew[c] = yv[c];
            if (io.seq_out && mode != ND_HEAD_GIVEN) ND_GW(io.seq_out)[z * io.seq_ms + ((size_t)i_step * M + m) * C + c] = yv[c];
        }
    }
    if (!live) return;
    float4 h;
    h.x = nd_head_element<C>(w1[0], yv, yh, a.x, cc.x, xe.x);
    h.y = nd_head_element<C>(w1[1], yv, yh, a.y, cc.y, xe.y);
    h.z = nd_head_element<C>(w1[2], yv, yh, a.z, cc.z, xe.z);
    h.w = nd_head_element<C>(w1[3], yv, yh, a.w, cc.w, xe.w);
    if (mb.h16 == 2)
        nd_b9_store4(reinterpret_cast<bf16x8*>(mb.h1), F >> 5, m, n, h.x, h.y, h.z, h.w);
    else if (mb.h16)
        *(__attribute__((address_space(1))) f16x4*)(reinterpret_cast<_Float16*>(mb.h1) + nd_pkh(m, n, F >> 5)) =
            f16x4{(_Float16)h.x, (_Float16)h.y, (_Float16)h.z, (_Float16)h.w};
    else
        *(__attribute__((address_space(1))) f32x4*)(mb.h1 + nd_pk(m, n, nchF)) = f32x4{h.x, h.y, h.z, h.w};
}

// Step head of the LDS-tiled blocks (M > 128 rows, h1 a frag32b3 image): k_step_head's arithmetic -- per element, and in the eps
// reduction tree: NT <= 64 partials are one value per lane of a 64-lane shuffle tree there, four values per lane of a 16-lane tree
// here, paired the same way, so both kernels return the same bits -- laid out for many rows.  A workgroup takes 16 rows x
// ND_HEAD_ROWS_COLS columns: it reduces eps and updates y for its rows ONCE (k_step_head: a workgroup per row and 1024 columns), and every lane
// computes the 8 consecutive k of one row that are its 16 bytes of an MFMA operand plane, so a wave writes whole 1 KiB planes of
// the image (k_step_head's 8-byte pieces land 256 bytes apart).
// Grid (ceil(F/ND_HEAD_ROWS_COLS), ceil(M/16), members), 256 threads; F % 32 == 0, NT <= 64.
template <int C, bool COEF = false>
__global__ __launch_bounds__(256) void k_step_head_rows(MemberInline mi, const MemberDev* __restrict__ members, StepIO io, int mode,
                                                        int i_step, int t_prev, int t, int B, int M, int maxM, int F, int NT, int T) {
    typedef const __attribute__((address_space(4))) char* nd_cbytes;
    const MemberDev mb = nd_ldc<MemberDev>((members ? (nd_cbytes)(uintptr_t)members : (nd_cbytes)__builtin_amdgcn_kernarg_segment_ptr()) +
                                           (size_t)blockIdx.z * sizeof(MemberDev));
    const int z = blockIdx.z, tid = threadIdx.x, m0 = blockIdx.y * 16;
    constexpr int C2 = 2 * C;
    __shared__ float ys[16][C], yhs[16][C];
    {   // thread (r = tid / 16, j = tid % 16) holds partials j, j + 16, j + 32, j + 48 of row m0 + r
        const int r = tid >> 4, j = tid & 15, m = min(m0 + r, M - 1), b = m % B;
        const int par_new = i_step & 1;
        nd_gf ynew = ND_GW(mb.ybuf + ((size_t)par_new * maxM + m) * C);
        nd_gcf yold = ND_GC(mb.ybuf + ((size_t)(par_new ^ 1) * maxM + m) * C);
        float yv[C], yh[C], ym[C], zz[C], yo[C], eps[C];
        float al = 0.f, s_t = 0.f, s_tm1 = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            yh[c] = ND_GC(io.yhat)[z * io.yhat_ms + (size_t)b * C + c];
            eps[c] = 0.f; ym[c] = 0.f; zz[c] = 0.f; yo[c] = 0.f;
        }
        if (mode != ND_HEAD_GIVEN) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                ym[c] = ND_GC(io.ymean)[z * io.ymean_ms + (size_t)b * C + c];
                zz[c] = ND_GC(io.noise)[z * io.noise_ms + ((size_t)i_step * M + m) * C + c];
            }
        }
        float cf[4] = {0.f, 0.f, 0.f, 0.f};
        if (mode == ND_HEAD_UPDATE) {
            if constexpr (COEF) {
#pragma unroll
                for (int q = 0; q < 4; ++q) cf[q] = ND_GC(io.alphas)[4 * t_prev + q];
            } else {
                al = ND_GC(io.alphas)[t_prev]; s_t = ND_GC(io.omabs)[t_prev]; s_tm1 = ND_GC(io.omabs)[t_prev - 1];
            }
#pragma unroll
            for (int c = 0; c < C; ++c) {
                yo[c] = yold[c];
                nd_gcf row = ND_GC(mb.epart + ((size_t)m * C + c) * NT);
                // nd_reduce_eps<256, C> at NT <= 64: lane i of wave 0 starts from 0.f + row[i] (0.f past NT); shuffle steps 32 and 16
                // pair (i, i+32) and then (i, i+16); steps 8..1 follow below; the other three waves add 0.f each
                float q[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int tl = j + 16 * k;
                    const float v = row[min(tl, NT - 1)];
                    q[k] = tl < NT ? 0.f + v : 0.f;
                }
                float s = (q[0] + q[2]) + (q[1] + q[3]);
#pragma unroll
                for (int off = 8; off > 0; off >>= 1) s += __shfl_down(s, off, 16);
                float tot = 0.f;
                tot += s;
                tot += 0.f; tot += 0.f; tot += 0.f;
                eps[c] = __shfl(tot, 0, 16);
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            if (mode == ND_HEAD_INIT) yv[c] = zz[c] + ym[c];
            else if (mode == ND_HEAD_UPDATE)
                yv[c] = COEF ? nd_coef_update(yo[c], ym[c], eps[c] + ND_GC(mb.lin4_b)[c], zz[c], cf[0], cf[1], cf[2], cf[3])
                             : nd_posterior(yo[c], ym[c], eps[c] + ND_GC(mb.lin4_b)[c], zz[c], al, s_t, s_tm1);
            else yv[c] = ND_GC(io.y_in)[z * io.yin_ms + (size_t)m * C + c];
            if (j == 0) {
                ys[r][c] = yv[c]; yhs[r][c] = yh[c];
                if (blockIdx.x == 0 && m0 + r < M) {
                    ynew[c] = yv[c];
                    if (io.seq_out && mode != ND_HEAD_GIVEN) ND_GW(io.seq_out)[z * io.seq_ms + ((size_t)i_step * M + m) * C + c] = yv[c];
                }
            }
        }
    }
    __syncthreads();
    // lane l of a wave: row m0 + (l & 15), the 8 columns kq = l >> 4 of each 32-column block -> its 16 bytes of the three planes
    const int lane = tid & 63, wave = tid >> 6, r = lane & 15, kq = lane >> 4;
    const int m = m0 + r, b = min(m, M - 1) % B, nkb = F >> 5, nchF = F >> 4;
    float yv[C], yh[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { yv[c] = ys[r][c]; yh[c] = yhs[r][c]; }
    bf16x8* img = reinterpret_cast<bf16x8*>(mb.h1);
#pragma unroll
    for (int it = 0; it < ND_HEAD_ROWS_COLS / 128; ++it) {
        const int kb = blockIdx.x * (ND_HEAD_ROWS_COLS / 32) + wave * (ND_HEAD_ROWS_COLS / 128) + it;
        if (kb >= nkb) break;
        const int n = kb * 32 + kq * 8;
        const float4 a0 = nd_ld16<false>(mb.A1 + (size_t)t * F + n), a1 = nd_ld16<false>(mb.A1 + (size_t)t * F + n + 4);
        const float4 c0 = nd_ld16<false>(mb.C1 + (size_t)t * F + n), c1 = nd_ld16<false>(mb.C1 + (size_t)t * F + n + 4);
        const float4 x0 = nd_ld16<false>(mb.xe + nd_pk(b, n, nchF)), x1 = nd_ld16<false>(mb.xe + nd_pk(b, n + 4, nchF));
        const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
        const float cv[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
        const float xv[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
        nd_gcf wrow = ND_GC(mb.lin1_w + (size_t)n * C2);       // 8 consecutive rows = 8*C2 contiguous floats
        float w1[8][C2];
#pragma unroll
        for (int jj = 0; jj < 8; ++jj)
#pragma unroll
            for (int q = 0; q < C2; ++q) w1[jj][q] = wrow[jj * C2 + q];
        bf16x8 p1, p2, p3;
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
            const float hv = nd_head_element<C>(w1[jj], yv, yh, av[jj], cv[jj], xv[jj]);
            __bf16 e1, e2, e3;
            nd_b9_split(hv, e1, e2, e3);
            p1[jj] = e1; p2[jj] = e2; p3[jj] = e3;
        }
        if (m < M) {
            __attribute__((address_space(1))) bf16x8* q = (__attribute__((address_space(1))) bf16x8*)(img + ((size_t)(m0 >> 4) * nkb + kb) * B9_BLOCK_UNITS + lane);
            q[0] = p1; q[64] = p2; q[128] = p3;
        }
    }
}

// Last step (t = 0): y_0 = y_0_reparam (diffusion_utils.py:96-111), or plain eps output for the
// eps_theta entry point.  Grid (M, 1, members), 64 threads.
// eps_only: 0 = y_0 of the loop, 1 = eps output, 2 = one p_sample step from io.y_in with the draw in
// io.noise (t = par_cur), 3 = p_sample_t_1to0 from io.y_in.
// COEF: y_0 of the loop (eps_only 0) is nd_coef_update with row 0 of the plan's table (io.alphas): its cz is 0 and no draw is read.
template <int C, bool COEF = false>
__global__ __launch_bounds__(64) void k_step_final(MemberInline mi, const MemberDev* __restrict__ members, StepIO io, int eps_only, int par_cur,
                                                   int B, int M, int maxM, int NT, int T, float* eps_out, size_t eps_ms) {
    typedef const __attribute__((address_space(4))) char* nd_cbytes;           // scalar loads from either source (see k_skinny)
    const MemberDev mb = nd_ldc<MemberDev>((members ? (nd_cbytes)(uintptr_t)members : (nd_cbytes)__builtin_amdgcn_kernarg_segment_ptr()) +
                                           (size_t)blockIdx.z * sizeof(MemberDev));
    const int z = blockIdx.z, m = blockIdx.x, b = m % B;
    __shared__ float red[C];
    float epsv[C];
    nd_reduce_eps<64, C>(mb.epart, NT, m, red, epsv);
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float eps = epsv[c] + mb.lin4_b[c];
        if (threadIdx.x == 0) {
            if (eps_only == 1) {
                eps_out[z * eps_ms + (size_t)m * C + c] = eps;
            } else if (eps_only >= 2) {
                const float y = io.y_in[(size_t)m * C + c];
                const float ymean = io.ymean[(size_t)b * C + c];
                const int t = par_cur;
                eps_out[(size_t)m * C + c] = eps_only == 2
                    ? nd_posterior(y, ymean, eps, io.noise[(size_t)m * C + c], io.alphas[t], io.omabs[t], io.omabs[t - 1])
                    : nd_y0_reparam(y, ymean, eps, io.omabs[0]);
            } else {
                const float y = mb.ybuf[((size_t)par_cur * maxM + m) * C + c];
                const float ymean = io.ymean[z * io.ymean_ms + (size_t)b * C + c];
                const float y0 = COEF ? nd_coef_update(y, ymean, eps, 0.f, io.alphas[0], io.alphas[1], io.alphas[2], io.alphas[3])
                                      : nd_y0_reparam(y, ymean, eps, io.omabs[0]);
                io.y0_out[z * io.y0_ms + (size_t)m * C + c] = y0;
                if (io.seq_out) io.seq_out[z * io.seq_ms + ((size_t)T * M + m) * C + c] = y0;
            }
        }
    }
}

// the instantiation of kernel template K for y_dim = C (the entry points admit 1 .. ND_MAX_C = 8 only)
#define ND_KERNEL_BY_C(K, C)                                                                                            \
    ((C) == 1 ? (void*)K<1> : (C) == 2 ? (void*)K<2> : (C) == 3 ? (void*)K<3> : (C) == 4 ? (void*)K<4> : (C) == 5 ? (void*)K<5> \
   : (C) == 6 ? (void*)K<6> : (C) == 7 ? (void*)K<7> : (void*)K<8>)

#define ND_COEF_KERNEL_BY_C(K, C)                                                                                                \
    ((C) == 1 ? (void*)K<1, true> : (C) == 2 ? (void*)K<2, true> : (C) == 3 ? (void*)K<3, true> : (C) == 4 ? (void*)K<4, true>       \
   : (C) == 5 ? (void*)K<5, true> : (C) == 6 ? (void*)K<6, true> : (C) == 7 ? (void*)K<7, true> : (void*)K<8, true>)

void* nd_step_head_kernel(int C, bool rows, bool coef) {
    if (coef) return rows ? ND_COEF_KERNEL_BY_C(k_step_head_rows, C) : ND_COEF_KERNEL_BY_C(k_step_head, C);
    return rows ? ND_KERNEL_BY_C(k_step_head_rows, C) : ND_KERNEL_BY_C(k_step_head, C);
}
void* nd_step_final_kernel(int C, bool coef) { return coef ? ND_COEF_KERNEL_BY_C(k_step_final, C) : ND_KERNEL_BY_C(k_step_final, C); }
