// nd_host.hpp -- the host prelude of every translation unit of libnd_hip.so: the error plumbing and the pointer checks of the entry points.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/nested_diffusion.h"

// records the message nd_last_error() returns and hands `code` back (defined in nd_error.hip)
int nd_set_err(int code, const char* fmt, ...);

// (a macro: __FILE__ and __LINE__ name the call that failed)
#define HIP_CHECK(expr)                                                                              \
    do {                                                                                             \
        hipError_t _e = (expr);                                                                      \
        if (_e != hipSuccess)                                                                        \
            return nd_set_err(ND_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

// operand dtype of the Linear / GEMM / attention entry points, and the K multiple of its MFMA (16x16x4 f32, 16x16x32 f16)
inline int nd_bad_dtype(int dtype) { return dtype != ND_DTYPE_F32 && dtype != ND_DTYPE_F16; }
inline int nd_kmul(int dtype) { return dtype == ND_DTYPE_F16 ? 32 : 16; }

// workgroups of 256 threads for `items` work items: ceil(items / 256), at least 1, at most cap (grid-stride beyond)
inline unsigned nd_blocks_per_image(size_t items, unsigned cap) {
    const size_t per = (items + 255) / 256;
    return (unsigned)(per > cap ? cap : (per ? per : 1));
}

inline bool nd_misaligned(const void* p, uintptr_t mask) { return ((uintptr_t)p & mask) != 0; }

// true when two of the non-NULL pointers are the same buffer
inline bool nd_any_equal(const void* const* p, int n) {
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j)
            if (p[i] && p[i] == p[j]) return true;
    return false;
}
