// nd_device.hpp -- what a launch plan asks the current device: its compute-unit count, and leave to use more than 64 KiB of dynamic LDS.
// Host only; one instance of each cache for the whole library (inline functions).
#pragma once
#include <mutex>
#include <unordered_map>
#include <hip/hip_runtime.h>

// Compute units of the CURRENT device (256 on an MI355X in SPX mode, fewer under CPX partitioning), queried once per
// device.  Launch geometry is a pure function of (shape, CU count); 256 is assumed when no device is visible (host-only
// plan introspection in the build container).
inline int nd_num_cus() {
    static int cached[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (cached[dev] == 0) {
        int n = 0;
        cached[dev] = (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : 256;
    }
    return cached[dev];
}

// A kernel that asks for more than 64 KiB of dynamic LDS has to be told so before its first launch (graph kernel nodes included), and
// hipFuncSetAttribute is PER DEVICE: remembered as one bit per device and kernel (devices beyond 63: set every time).  One table for the
// whole library (inline function: one instance across translation units); failures are returned, never cached.
inline hipError_t nd_allow_dynamic_lds(const void* fn, size_t bytes) {
    static std::mutex mu;
    static std::unordered_map<const void*, unsigned long long> done;      // kernel -> devices that have the attribute
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> g(mu);
    unsigned long long& mask = done[fn];
    if (dev >= 0 && dev < 64 && ((mask >> dev) & 1ull)) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess && dev >= 0 && dev < 64) mask |= 1ull << dev;
    return e;
}
