// nd_rng.hpp -- the kernels of the in-library noise generator (nd_rng.hip) for the sampler's translation unit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// kernel handles for hipLaunchKernel / hipGraph kernel nodes; argument lists:
//   philox:  (float* out, const unsigned long long* state, unsigned long long seed, uint32_t batch, uint32_t first, int m0, int nm, int T, int B, int mc, int C)
//            out[nm][T][mc*B][C] standard normals for ensemble members m0 .. m0+nm-1 (the member word of the counter is m0 + k).
//            state != nullptr: {seed, batch counter | first image << 32} is read on the DEVICE at run time (hipGraph replays see the
//            current values); else the three scalar arguments are used.  Grid nd_philox_normal_grid(...), block 256
//   advance: (unsigned long long* state), grid 1, block 64: batch counter += 1 (last kernel of a sampling call)
void* nd_philox_normal_kernel();
void* nd_rng_advance_kernel();
// one thread per (member, draw, row, class-quad)
inline dim3 nd_philox_normal_grid(int nm, int T, int B, int mc, int C) {
    const size_t total = (size_t)nm * T * B * mc * ((C + 3) / 4);
    return dim3((unsigned)((total + 255) / 256));
}
