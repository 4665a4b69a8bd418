// nd_attack.hpp -- what the three attack units (nd_attack_linf.hip, nd_attack_l2.hip, nd_square.hip) share: the clamp of their
// elementwise passes, the argument check of "B images of per_image elements" and the (workgroups per image, images) grid.
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
