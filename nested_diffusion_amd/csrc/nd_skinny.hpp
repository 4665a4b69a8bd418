// nd_skinny.hpp -- what a caller of the weight-streaming kernel k_skinny needs: the member descriptors, the launch plan and the launch
// helpers, and the split-K epilogue's descriptor and launcher.  The kernel itself and the plan's body: nd_skinny_kernel.hpp, instantiated
// by csrc/nd_skinny_m{0,1,2}.hip only.  Operand layouts: nd_frag.hpp.  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>

// One skinny Linear on packed operands, for `nm` members that share the layer shape (K, N):
//   MODE 0: out[m,n] = act(scale[t,n] * sum_k x[m,k] w[n,k] + shift[t,n])
//   MODE 1: that value is not stored; its projection onto C rows is: part[m,c,tile] = sum_{n in tile} pw[c,n]*v
//           -- lin3 + unetnorm3 + softplus + lin4 (latent_model.py:181-184) in one pass.
//   MODE 2: split-K partial sums, no epilogue: part[slab, m, n] = sum_{k in slab} x[m,k] w[n,k]
struct SkinnyDesc {
    const float* x;      // frag16 [M][K]   (frag32h in the fp16 kernels: opaque 1 KiB blocks either way)
    const float* w;      // frag16 [N][K]   (nn.Linear weight, rows padded to 16 with zeros)
    const float* scale;  // [rows, N] or nullptr (=1)
    const float* shift;  // [rows, N] or nullptr (=0)
    float* out;          // MODE 0: out_packed 0 = row-major fp32 [M][N], 1 = frag16 fp32, 2 = frag32h fp16 (N % 32 == 0)
    const float* pw;     // [C, N]            (MODE 1)
    float* part;         // MODE 1: [M, C, ceil(N/16)];  MODE 2: [S, Mpad, Npad]
    int K, N, C, act, out_packed;
    int keep;            // 1: this member's W is read with default-policy loads in an NT kernel (kept in the Infinity Cache across steps)
    const float* pf;     // or null: the weight matrix (same shape, same packing) of the NEXT launch of this member's step chain: near the end
                         // of its stream every wave touches the lines of the first register stage the same workgroup of that launch will ask
                         // for -- same blockIdx, hence same XCD and L2 -- so that launch's ramp starts on L2 hits instead of HBM latency
};

// Up to ND_INLINE_DESCS members' descriptors travel BY VALUE in the kernel arguments (table == nullptr): a workgroup then has its
// operand pointers after one scalar load from the kernarg segment instead of a kernarg load followed by a dependent global load
// of table[g] -- one memory round trip less before the first weight request of every launch.
#define ND_INLINE_DESCS 8
struct SkinnyInline { SkinnyDesc d[ND_INLINE_DESCS]; };

// Row fragments (16 rows each) per workgroup pass: 1, 2 or 4 -- and FIVE where that saves a whole pass over the weights: 65..80 rows
// (the reference's default batch of 70, configs/chest_x_ray.yml:66: one pass of 80 rows instead of two of 64), 129..160, ...
// Measured against 4 everywhere on one box (profiles/r04_rows5_ab.txt): B = 70, mc = 1: 546 k -> 794 k step*img/s (fp16 operands
// 1.50 M -> 2.12 M); fp16 operands at 640 rows (mc = 20): 4.76 M -> 5.33 M.
static inline int nd_pick_mt(int M) {
    if (M <= 16) return 1;
    if (M <= 32) return 2;
    const int f = (M + 15) / 16;
    return (f + 4) / 5 < (f + 3) / 4 ? 5 : 4;
}
static inline bool nd_use_splitk(int K) { return K >= 16384; }

// err: what preparing the launch returned (the dynamic-LDS attribute of the kernel on the current device); the launchers below hand it
// back instead of launching, so it reaches the caller through nd_set_err like any other HIP error
struct SkinnyLaunch { void* fn; dim3 grid; dim3 block; int cps; int S; unsigned lds; hipError_t err; };   // lds: dynamic LDS bytes of the launch

// The k_skinny family (4 row-fragment counts x 6 weight-fragment counts x 2 load policies x 2 operand types per MODE) is instantiated
// ONCE per MODE, each in a translation unit of its own (csrc/nd_skinny_m{0,1,2}.hip, from nd_skinny_kernel.hpp: the plan is
// nd_skinny_launch_impl there); every other translation unit gets its launch plan -- kernel pointer included -- through these three
// functions.
SkinnyLaunch nd_skinny_launch_m0(int K, int N, int M, int nm, int half);
SkinnyLaunch nd_skinny_launch_m1(int K, int N, int M, int nm, int half);
SkinnyLaunch nd_skinny_launch_m2(int K, int N, int M, int nm, int half);
template <int MODE>
static inline SkinnyLaunch nd_skinny_launch(int K, int N, int M, int nm, int half = 0) {
    return MODE == 0 ? nd_skinny_launch_m0(K, N, M, nm, half) : MODE == 1 ? nd_skinny_launch_m1(K, N, M, nm, half) : nd_skinny_launch_m2(K, N, M, nm, half);
}

static inline size_t nd_splitk_part_floats(int M, int K, int N, int nm = 1, int half = 0) {
    const SkinnyLaunch L = nd_skinny_launch<2>(K, N, M, nm, half);
    return (size_t)L.S * (size_t)(((M + 15) / 16) * 16) * (size_t)(((N + 15) / 16) * 16);
}

// descs: HOST copies of the nm members' descriptors (nm <= ND_INLINE_DESCS): passed by value
static inline hipError_t nd_launch_skinny_inline(const SkinnyLaunch& L, const SkinnyDesc* descs, int nm, int M, int t, hipStream_t st) {
    if (L.err != hipSuccess) return L.err;
    int cps = L.cps;
    SkinnyInline di{};
    for (int g = 0; g < nm && g < ND_INLINE_DESCS; ++g) di.d[g] = descs[g];
    const SkinnyDesc* table = nullptr;
    void* args[] = {&di, &table, &nm, &M, &t, &cps};
    return hipLaunchKernel(L.fn, L.grid, L.block, args, L.lds, st);
}

// d0: the descriptor of a single-member launch (table == nullptr, nm == 1), else ignored: table[0 .. nm) in device memory.
static inline hipError_t nd_launch_skinny(const SkinnyLaunch& L, SkinnyDesc d0, const SkinnyDesc* table, int nm, int M, int t,
                                          hipStream_t st) {
    if (L.err != hipSuccess) return L.err;
    int cps = L.cps;
    SkinnyInline di{};
    di.d[0] = d0;
    void* args[] = {&di, &table, &nm, &M, &t, &cps};
    return hipLaunchKernel(L.fn, L.grid, L.block, args, L.lds, st);
}

// ---- the split-K epilogue (kernel and launcher: csrc/nd_skinny_m2.hip) ----
// out[m,n] = act(scale[n] * sum_s part[s,m,n] + shift[n]); slabs summed in order (reproducible).
// One thread per 4 consecutive n; output frag16 (feeds the next skinny GEMM) or row-major.
struct SplitKEpiDesc {
    const float* part;   // [S, Mpad, Npad]
    const float* scale;  // [N] or nullptr
    const float* shift;  // [N] or nullptr
    float* out;          // frag16 [M][N] (N % 16 == 0) or row-major [M][N]
    int N, S, act, out_packed;
};

// one launch over [16*ceil(M/16)][16*ceil(N/16)] for nm members: table == nullptr (nm = 1) takes d0, else table[0 .. nm) in device memory
// (their N all equal to N).  csrc/nd_skinny_m2.hip.  The caller checks the launch (hipGetLastError).
void nd_launch_splitk_epilogue(SplitKEpiDesc d0, const SplitKEpiDesc* table, int nm, int M, int N, int S, hipStream_t st);
