// nd_error.hip -- the error plumbing of every translation unit of libnd_hip.so (nd_host.hpp) and the version string.  Host code only.
#include "nd_host.hpp"

#include <string>
#include <cstdio>
#include <cstdarg>

static thread_local std::string g_err;
extern "C" const char* nd_last_error(void) { return g_err.c_str(); }
extern "C" const char* nd_version(void) { return "libnd_hip gfx950 f32 (f32-input MFMA streams + bf16x9 exact-product GEMMs and attention) r6"; }
int nd_set_err(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
