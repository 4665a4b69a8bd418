// nd_attack.hpp -- what the attack units (nd_attack_linf.hip, nd_attack_l2.hip, nd_apgd_l2.hip, nd_square.hip) share: the clamp of their
// elementwise passes, the argument check of "B images of per_image elements", the (workgroups per image, images) grid and the
// fixed-shape row sum of the L2 units.
#pragma once
#include "nd_host.hpp"

constexpr int ND_ATTACK_THREADS = 256;      // the workgroup size nd_image_grid counts in

__device__ __forceinline__ float nd_clampf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// B images of per_image elements read as float4 quads: per_image % 4 == 0 and per_image / 4 <= max_quads (the kernel's int loop
// bound; the caller passes its own).  max_B is 65535 where the image is gridDim.y.  Runs before any HIP call.
inline int nd_check_rows(const char* what, int B, size_t per_image, int max_B, size_t max_quads) {
    if (B < 1 || B > max_B || per_image == 0 || (per_image % 4) || per_image / 4 > max_quads)
        return nd_set_err(ND_ERR_ARG, "%s needs 1 <= B <= %d and per_image %% 4 == 0 (B=%d, per_image=%zu)", what, max_B, B, per_image);
    return ND_OK;
}

// (workgroups per image, images): every workgroup belongs to one image; enough of them (nd_blocks_per_image, nd_host.hpp) to fill
// the chip at B = 1
static_assert(ND_ATTACK_THREADS == 256, "nd_blocks_per_image counts in workgroups of 256");
inline dim3 nd_image_grid(int B, size_t items, unsigned cap) { return dim3(nd_blocks_per_image(items, cap), (unsigned)B); }

// ---- the row sum of the L2 units (nd_attack_l2.hip, nd_apgd_l2.hip): grid (nd_l2_parts(per_image), B), workgroups of ND_ATTACK_THREADS;
// a thread sums its quads in grid-stride order, a workgroup folds its 256 threads with l2_block_sum and writes one partial, and the
// finishing pass (l2_finish) folds the <= 256 partials of an image with the same tree.  No floating-point atomics.

// the sum over the workgroup, the same bits in every thread (an xor butterfly adds the same two numbers in both partners)
__device__ __forceinline__ float l2_block_sum(float s, float* sh) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    __syncthreads();                                     // sh may still be read from a previous sum
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// the finishing pass: partials [parts] of one image (parts <= 256), folded by the same tree
__device__ __forceinline__ float l2_finish(const float* __restrict__ part, int parts, float* sh) {
    return l2_block_sum((int)threadIdx.x < parts ? part[threadIdx.x] : 0.f, sh);
}

// four products and three adds, each rounded: contraction is off here whatever the includer has set by this point
__device__ __forceinline__ float l2_sq4(float4 a) {
#pragma clang fp contract(off)
    return (a.x * a.x + a.y * a.y) + (a.z * a.z + a.w * a.w);
}
