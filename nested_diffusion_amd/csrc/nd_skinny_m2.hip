// nd_skinny_m2.hip -- the k_skinny<..., MODE 2, ...> family: split-K: raw partial sums per k-slab, finished by k_splitk_epilogue (encoder_x.0, mapping linear1).
// One translation unit per MODE (the three compile side by side; nd_skinny_kernel.hpp explains the kernel and the launch plan).  gfx950 only.
#include "nd_skinny_kernel.hpp"

SkinnyLaunch nd_skinny_launch_m2(int K, int N, int M, int nm, int half) { return nd_skinny_launch_impl<2>(K, N, M, nm, half); }

// ---- the split-K epilogue (SplitKEpiDesc, nd_skinny.hpp): what finishes the partial sums of the launches planned above ----
__global__ __launch_bounds__(256) void k_splitk_epilogue(SplitKEpiDesc d0, const SplitKEpiDesc* __restrict__ table, int M, int S) {
    const SplitKEpiDesc d = table ? table[blockIdx.z] : d0;
    const int N = d.N, Np = ((N + 15) >> 4) * 16, Mp = ((M + 15) >> 4) * 16;
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;   // float4 index over [Mp][Np]
    if (q >= (size_t)Mp * Np / 4) return;
    const int m = (int)(q / (Np / 4)), n = (int)(q % (Np / 4)) * 4;
    const size_t slab = (size_t)Mp * Np;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k < S; ++k) {
        const float4 v = *reinterpret_cast<const float4*>(d.part + (size_t)k * slab + (size_t)m * Np + n);
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    float o[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int nn = min(n + r, N - 1);
        const float a = d.scale ? d.scale[nn] : 1.0f;
        const float b = d.shift ? d.shift[nn] : 0.0f;
        o[r] = (n + r < N) ? nd_act(a * o[r] + b, d.act) : 0.f;
    }
    if (d.out_packed == 2) {
        *reinterpret_cast<f16x4*>(reinterpret_cast<_Float16*>(d.out) + nd_pkh(m, n, N >> 5)) =
            f16x4{(_Float16)o[0], (_Float16)o[1], (_Float16)o[2], (_Float16)o[3]};
    } else if (d.out_packed) {
        *reinterpret_cast<float4*>(d.out + nd_pk(m, n, N >> 4)) = make_float4(o[0], o[1], o[2], o[3]);
    } else if (m < M) {
#pragma unroll
        for (int r = 0; r < 4; ++r) if (n + r < N) d.out[(size_t)m * N + n + r] = o[r];
    }
}

void nd_launch_splitk_epilogue(SplitKEpiDesc d0, const SplitKEpiDesc* table, int nm, int M, int N, int S, hipStream_t st) {
    const size_t q = (size_t)(((M + 15) / 16) * 16) * (((N + 15) / 16) * 16) / 4;      // float4 pieces of one member's padded output
    hipLaunchKernelGGL(k_splitk_epilogue, dim3((unsigned)((q + 255) / 256), 1, nm), dim3(256), 0, st, d0, table, M, S);
}

#ifdef ND_WG_TIMING
// debug builds only (tools/wg_times.py): this translation unit's copy of the clock buffer pointer
int nd_debug_set_wg_times_m2(void* dev_ptr) { return hipMemcpyToSymbol(HIP_SYMBOL(nd_dbg_times), &dev_ptr, sizeof dev_ptr) == hipSuccess ? 0 : -1; }
// ... and the entry point that sets all three: where k_skinny drops its per-workgroup clocks, 3 x 8192 x 3 int64
int nd_debug_set_wg_times_m0(void*); int nd_debug_set_wg_times_m1(void*);
extern "C" int nd_debug_set_wg_times(void* dev_ptr) {
    return (nd_debug_set_wg_times_m0(dev_ptr) | nd_debug_set_wg_times_m1(dev_ptr) | nd_debug_set_wg_times_m2(dev_ptr)) ? -1 : 0;
}
#endif
