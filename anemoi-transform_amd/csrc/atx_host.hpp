// Host-side plumbing shared, as source, by the nine libraries (libatx, libatx_text, libatx_plan, libatx_mesh, libatx_missing,
// libatx_stat, libatx_levels, libatx_geopotential, libatx_heights): the
// calling thread's error message, the require-and-return macros and the grid of a one-lane-per-item launch.  Host code only, so a
// companion library includes it without atx_common.hpp's device helpers.
//
// The message cell is ONE PER LIBRARY and per thread: last_error() is an inline function with a function-local static, every object
// is compiled with -fvisibility=hidden and every library links under a version script that ends in `local: *`, so the translation
// units of one library share the cell and no two libraries do (tests/test_native_messages.py).  Each library's *_last_error entry
// point returns last_error().c_str().
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdarg>
#include <cstdio>
#include <string>

#include "../../include/atx.h"

namespace atx {

inline std::string& last_error() {
    static thread_local std::string cell;
    return cell;
}

inline void set_error(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    last_error() = buf;
}

inline int hip_status(hipError_t e, const char* what) {
    if (e == hipSuccess) return ATX_OK;
    set_error("%s: HIP error %d (%s)", what, (int)e, hipGetErrorString(e));
    return ATX_EHIP;
}

#define ATX_REQUIRE(cond, code, ...)  \
    do {                              \
        if (!(cond)) {                \
            atx::set_error(__VA_ARGS__); \
            return (code);            \
        }                             \
    } while (0)

#define ATX_LAUNCH_CHECK(what)                                   \
    do {                                                         \
        int _st = atx::hip_status(hipGetLastError(), what);      \
        if (_st != ATX_OK) return _st;                           \
    } while (0)

// Workgroups of `block` lanes for n items, one lane each, at most `cap` of them (a grid-stride kernel takes the rest).
inline unsigned grid_for(int64_t n, int block, int64_t cap) {
    const int64_t blocks = (n + block - 1) / block;
    return (unsigned)(blocks < cap ? blocks : cap);
}

}  // namespace atx
