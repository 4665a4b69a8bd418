// nd_mlp_grad.hip -- the gradient through the mapping MLPs (include/nested_diffusion.h: nd_linear_bwd, nd_ensemble_xent_bwd; the chain:
// nested_diffusion_amd/mapping.py GuidingConditioner.input_grad).  gfx950 only, all arithmetic fp32.
//   k_linear_bwd          out[M, K] = ((dy[M, N] . W[N, K]) (.) (gate > 0)) + add, W read in place from its nd_pack_rows (frag16) image
//   k_ensemble_xent_bwd   cross-entropy of the members' averaged softmax: P, per-image loss and every member's dlogits
//
// k_linear_bwd.  The forward stream (nd_linear) contracts over K, the direction the frag16 image is laid out for: lane l of a wave loads
// W[n = l & 15][k = 4 (l >> 4) + j] of a 1 KiB block and that float4 is directly an MFMA operand.  The input gradient contracts over n, the
// image's ROWS.  v_mfma_f32_16x16x4_f32 wants the contracted index in l >> 4 on both operands, so each block is transposed once between
// the load and the MFMA, through LDS: a wave writes its float4 to slot 16 q + (n ^ q) (q = l >> 4: the xor spreads the later column reads
// over all banks), then lane l reads W[n = 4 (l >> 4) + j][k = l & 15] for j = 0..3.  The dy operand needs no transpose: loaded in frag16
// order (lane l: dy[m = l & 15][n = 4 (l >> 4) + j]), MFMA j contracts n in {j, 4 + j, 8 + j, 12 + j} of the row block on both sides.
//
// Work split: a wave owns LB_KBW adjacent 16-column blocks and walks ALL row blocks rb = 0 .. ceil(N / 16) - 1 for them, so its HBM reads
// are contiguous LB_KBW KiB pieces (the four waves of a workgroup sit side by side: 4 * LB_KBW KiB), K / 16 KiB apart from one row block to
// the next.  Nothing is split over the contraction: no atomics, no second pass, no workspace.  An output element is one chain over
// rb ascending, j = 0..3 inside a row block, whatever M is and whichever rows share the launch (an MFMA's output rows do not mix), so a
// row's result has the same bits in any batch and on every run.
// Rows n >= N of the image are the zero padding of nd_pack_rows; their dy operand is zero-filled in registers, never read (0 * garbage
// would be NaN), and so are the rows m >= M of the last 16-row tile.
#include "nd_frag.hpp"
#include "nd_host.hpp"

namespace {

constexpr int LB_WAVES = 4;       // waves per workgroup
constexpr int LB_KBW = 4;         // adjacent 16-column blocks per wave: one contiguous 4 KiB read per row block
constexpr int LB_DEPTH = 2;       // register stages of (dy, weight) loads per wave: one row block in flight beyond the one consumed; the sweep: EXPERIMENTS #45

// the dy fragment of row tile mt and row block rb: lane l holds dy[mt * 16 + (l & 15)][rb * 16 + 4 (l >> 4) + j], zero outside [M, N)
template <bool VEC>
__device__ __forceinline__ float4 lb_load_dy(const float* __restrict__ dy, int m, int n0, int M, int N) {
    if (VEC) {   // N % 4 == 0 and a 16-byte aligned base: a quad is inside the row or wholly past it.  Branch-free: a clamped (valid) address, then the select
        const int mc = m < M ? m : M - 1, nc = n0 < N ? n0 : N - 4;
        const float4 v = *reinterpret_cast<const float4*>(dy + (size_t)mc * N + nc);
        return (m < M && n0 < N) ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (m < M) {
        const float* p = dy + (size_t)m * N + n0;
        if (n0 + 0 < N) a.x = p[0];
        if (n0 + 1 < N) a.y = p[1];
        if (n0 + 2 < N) a.z = p[2];
        if (n0 + 3 < N) a.w = p[3];
    }
    return a;
}

template <int MT, bool VEC>
__global__ __launch_bounds__(LB_WAVES * 64) void k_linear_bwd(const float* __restrict__ dy, const float* __restrict__ w, const float* __restrict__ gate,
                                                             const float* add, float* out, int M, int N, int K) {
    __shared__ float4 lds[LB_WAVES][LB_KBW][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nkb = K >> 4, nrb = (N + 15) >> 4;
    const int kb0 = ((int)blockIdx.x * LB_WAVES + wave) * LB_KBW;
    if (kb0 >= nkb) return;                          // a whole wave past the last column block (no workgroup barrier below)
    const int nb = nkb - kb0 < LB_KBW ? nkb - kb0 : LB_KBW;
    const int q = lane >> 4, c = lane & 15;
    float4 (*my)[64] = lds[wave];

    f32x4 acc[MT][LB_KBW];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < LB_KBW; ++i) acc[mt][i] = f32x4{0.f, 0.f, 0.f, 0.f};

    const float* wp = w + (size_t)kb0 * 256 + (size_t)lane * 4;
    const size_t rb_stride = (size_t)nkb * 256;
    // LB_DEPTH register stages of (MT dy fragments, LB_KBW weight blocks): the loads of row block rb + LB_DEPTH - 1 are issued before row
    // block rb is consumed, dy first, so that the counted wait in front of a stage leaves every later stage in flight.  Column blocks past
    // the image's last (i >= nb) and row blocks past its last re-read a valid block instead of branching; what they feed is never stored.
    float4 st[LB_DEPTH][LB_KBW], av[LB_DEPTH][MT];
    auto issue = [&](int s, int rb) {
        const int rbc = rb < nrb ? rb : nrb - 1;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) av[s][mt] = lb_load_dy<VEC>(dy, mt * 16 + c, rbc * 16 + 4 * q, M, N);
        const float* wn = wp + (size_t)rbc * rb_stride;
#pragma unroll
        for (int i = 0; i < LB_KBW; ++i) st[s][i] = nd_ld16<true>(wn + (size_t)(i < nb ? i : nb - 1) * 256);
    };
#pragma unroll
    for (int s = 0; s < LB_DEPTH - 1; ++s) issue(s, s);

    for (int rb0 = 0; rb0 < nrb; rb0 += LB_DEPTH) {
#pragma unroll
        for (int s = 0; s < LB_DEPTH; ++s) {
            const int rb = rb0 + s;
            if (rb >= nrb) break;
            issue((s + LB_DEPTH - 1) % LB_DEPTH, rb + LB_DEPTH - 1);

            // transpose through LDS: written as loaded (lane = (n, k-quad)), read as (n-quad, k)
#pragma unroll
            for (int i = 0; i < LB_KBW; ++i) my[i][16 * q + (c ^ q)] = st[s][i];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int i = 0; i < LB_KBW; ++i) {
                const float* blk = reinterpret_cast<const float*>(my[i]);
                float b[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int n = 4 * q + j, kq = c >> 2;              // W[n][k = c] sits in the float4 of (n, k-quad c >> 2), word c & 3
                    b[j] = blk[(16 * kq + (n ^ kq)) * 4 + (c & 3)];
                }
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    const float a4[4] = {av[s][mt].x, av[s][mt].y, av[s][mt].z, av[s][mt].w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[mt][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[j], b[j], acc[mt][i], 0, 0, 0);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();                           // the next row block's writes come after these reads
        }
    }

    // acc[mt][i][r] = (dy . W)[m = mt * 16 + 4 q + r][k = (kb0 + i) * 16 + c]
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < LB_KBW; ++i) {
            if (i >= nb) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = mt * 16 + 4 * q + r;
                if (m >= M) continue;
                const size_t o = (size_t)m * K + (size_t)(kb0 + i) * 16 + c;
                float v = acc[mt][i][r];
                if (gate) v = gate[o] > 0.f ? v : 0.f;                 // ReLU'(0) = 0, a NaN gate gives 0
                if (add) v += add[o];
                out[o] = v;
            }
        }
}

template <int MT>
void lb_launch(bool vec, dim3 grid, hipStream_t st, const float* dy, const float* w, const float* gate, const float* add, float* out, int M, int N,
               int K) {
    if (vec) hipLaunchKernelGGL((k_linear_bwd<MT, true>), grid, dim3(LB_WAVES * 64), 0, st, dy, w, gate, add, out, M, N, K);
    else hipLaunchKernelGGL((k_linear_bwd<MT, false>), grid, dim3(LB_WAVES * 64), 0, st, dy, w, gate, add, out, M, N, K);
}

// ---------------------------------------------------------------------------------------------
// The ensemble's loss head.  One workgroup per image b.  Wave w takes the members k = w, w + 4, ...: the row maximum (a NaN never wins)
// and sum_c exp(l - max), lanes in stride-64 order folded by an xor butterfly; a NaN logit makes the member's sum, hence the whole row, NaN.
// Then every thread forms p_k[b, c] = exp(l - max_k) / sum_k for its columns, P = (sum_k p_k) / K in member order, and with labels
// S = sum_k p_k[b, y] in member order, loss = -logf(S / K) (the bits of -logf(P[b, y])) and dlogits_k = (p_k[b, y] / S) (p_k - [c == y]).
// One member (K == 1) is the plain softmax cross-entropy and is formed as a log-softmax, as torch's nn.CrossEntropyLoss is:
// loss = logf(sum) - (l_y - max) and dlogits = p - [c == y], no division by S.  p[b, y] may underflow there (a confidently wrong
// training sample, the label 104 or more behind the leading logit): the loss is then the margin and the gradient at the label -1, not
// +inf and 0 -- the S == 0 convention below is the ensemble's (K >= 2) alone.
// ---------------------------------------------------------------------------------------------
constexpr int EX_MAXK = 32;

__global__ __launch_bounds__(256) void k_ensemble_xent_bwd(const float* __restrict__ logits, const int64_t* __restrict__ labels, float* __restrict__ P,
                                                           float* __restrict__ loss, float* __restrict__ dlogits, int K, int B, int C) {
    __shared__ float s_mx[EX_MAXK], s_sum[EX_MAXK], s_py[EX_MAXK];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const size_t kstride = (size_t)B * C;
    const float* lb = logits + (size_t)b * C;
    for (int k = wave; k < K; k += 4) {
        const float* l = lb + (size_t)k * kstride;
        float mx = -INFINITY;
        for (int c = lane; c < C; c += 64) mx = fmaxf(mx, l[c]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
        float s = 0.f;
        for (int c = lane; c < C; c += 64) s += expf(l[c] - mx);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        if (lane == 0) { s_mx[k] = mx; s_sum[k] = s; }
    }
    __syncthreads();
    const bool have = labels != nullptr;
    const int64_t y = have ? labels[b] : -1;
    const bool valid = y >= 0 && y < C;
    if (have && valid && t < K) s_py[t] = expf(lb[(size_t)t * kstride + y] - s_mx[t]) / s_sum[t];
    __syncthreads();
    float S = 0.f;
    if (have && valid)
        for (int k = 0; k < K; ++k) S += s_py[k];
    const bool one = K == 1;                               // the plain cross-entropy: a log-softmax, which has no underflow to report
    if (have && t == 0) loss[b] = !valid ? NAN : one ? logf(s_sum[0]) - (lb[y] - s_mx[0]) : -logf(S / (float)K);
    const bool live = have && valid && (one || S != 0.f);  // K >= 2, S == 0 (underflow): loss = +inf above, no gradient; S NaN: NaN everywhere
    for (int c = t; c < C; c += 256) {
        float ps = 0.f;
        for (int k = 0; k < K; ++k) {
            const float p = expf(lb[(size_t)k * kstride + c] - s_mx[k]) / s_sum[k];
            ps += p;
            const float d = p - (c == y ? 1.0f : 0.0f);
            if (have) dlogits[(size_t)k * kstride + (size_t)b * C + c] = !live ? 0.f : one ? d : (s_py[k] / S) * d;
        }
        P[(size_t)b * C + c] = ps / (float)K;
    }
}

}  // namespace

extern "C" int nd_linear_bwd(const float* dy, const void* w_packed, const float* gate, const float* add, float* out, int M, int N, int K,
                             int dtype, void* stream) {
    if (!dy || !w_packed || !out) return nd_set_err(ND_ERR_ARG, "NULL tensor");
    if (dtype != ND_DTYPE_F32)
        return nd_set_err(ND_ERR_ARG, "linear_bwd reads fp32 (frag16) weight images only: the input gradient runs in fp32 mode, not on an fp16 image");
    if (M < 1 || M > ND_LINEAR_BWD_MAX_M) return nd_set_err(ND_ERR_ARG, "linear_bwd needs 1 <= M <= %d (M=%d)", ND_LINEAR_BWD_MAX_M, M);
    if (N < 1 || K < 16 || K % 16) return nd_set_err(ND_ERR_ARG, "linear_bwd needs N >= 1 and K a positive multiple of 16 (N=%d, K=%d)", N, K);
    if (((uintptr_t)w_packed & 15) || ((uintptr_t)dy & 3) || ((uintptr_t)out & 3) || ((uintptr_t)gate & 3) || ((uintptr_t)add & 3))
        return nd_set_err(ND_ERR_ARG, "misaligned tensor (the image 16 bytes, dy / gate / add / out 4)");
    const int nkb = K / 16, per_wg = LB_WAVES * LB_KBW;
    const dim3 grid((unsigned)((nkb + per_wg - 1) / per_wg));
    const bool vec = N % 4 == 0 && ((uintptr_t)dy & 15) == 0;
    const float* w = (const float*)w_packed;
    hipStream_t st = (hipStream_t)stream;
    const int tiles = (M + 15) / 16;
    if (tiles <= 1) lb_launch<1>(vec, grid, st, dy, w, gate, add, out, M, N, K);
    else if (tiles <= 2) lb_launch<2>(vec, grid, st, dy, w, gate, add, out, M, N, K);
    else if (tiles <= 4) lb_launch<4>(vec, grid, st, dy, w, gate, add, out, M, N, K);
    else lb_launch<8>(vec, grid, st, dy, w, gate, add, out, M, N, K);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_ensemble_xent_bwd(const float* logits, const int64_t* labels, float* P, float* loss, float* dlogits, int K, int B, int C,
                                    void* stream) {
    if (!logits || !P) return nd_set_err(ND_ERR_ARG, "NULL tensor");
    if (labels && (!loss || !dlogits)) return nd_set_err(ND_ERR_ARG, "labels need loss and dlogits");
    if (K < 1 || K > EX_MAXK || B < 1 || C < 2 || C > 1024)
        return nd_set_err(ND_ERR_ARG, "ensemble_xent_bwd needs 1 <= K <= %d, B >= 1 and 2 <= C <= 1024 (K=%d, B=%d, C=%d)", EX_MAXK, K, B, C);
    hipLaunchKernelGGL(k_ensemble_xent_bwd, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, logits, labels, P, loss, dlogits, K, B, C);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}
