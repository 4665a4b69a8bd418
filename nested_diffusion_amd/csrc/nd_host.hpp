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

inline bool nd_misaligned(const void* p, uintptr_t mask) { return ((uintptr_t)p & mask) != 0; }

// true when two of the non-NULL pointers are the same buffer
inline bool nd_any_equal(const void* const* p, int n) {
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j)
            if (p[i] && p[i] == p[j]) return true;
    return false;
}
