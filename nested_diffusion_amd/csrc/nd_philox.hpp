// nd_philox.hpp -- the one counter-based generator of the library (device only): Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel
// random numbers: as easy as 1, 2, 3", SC'11) and the two ways its 32-bit words become floats.  Every random draw of the package goes
// through these bodies (nd_rng.hip, nd_attack_linf.hip, nd_attack_l2.hip, nd_square.hip), so "an image draws the same numbers at any
// batch size, subset or rank" holds by construction; the host restatement the tests pin them to is oracle/ref_cpu.philox4x32_10.
//
// No multiply here feeds an add, so the bodies compile to the same code with and without `#pragma clang fp contract(off)` in the
// includer; the pragma stays in the translation units that need it and is not set here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ void nd_philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// two words -> two standard normals: u1 = (a + 1) * 2^-32, u2 = b * 2^-32, r = sqrt(-2 ln u1), (z0, z1) = r * (cos, sin)(2 pi u2)
__device__ __forceinline__ void nd_box_muller(uint32_t a, uint32_t b, float& z0, float& z1) {
    const float u1 = ((float)a + 1.0f) * 2.3283064365386963e-10f;       // (0, 1]: (2^32 - 1) + 1 rounds to 2^32 -> exactly 1
    const float u2 = (float)b * 2.3283064365386963e-10f;                 // [0, 1]
    const float r = sqrtf(-2.0f * logf(u1));
    float s, c;
    sincospif(2.0f * u2, &s, &c);
    z0 = r * c;
    z1 = r * s;
}

// one word -> a uniform in [0, 1) from its upper 24 bits: exact in fp32
__device__ __forceinline__ float nd_u24(uint32_t word) { return (float)(word >> 8) * 5.9604644775390625e-8f; }
