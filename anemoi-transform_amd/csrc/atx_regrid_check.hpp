// The argument checks of the gather entry points, once: the stack check and the ATX_VALIDATE range check of atx_regrid_ell /
// atx_regrid_csr (atx_regrid.hip), of atx_regrid_ell_missing / atx_regrid_csr_missing (missing/atx_regrid_missing.hip) and of
// atx_regrid_csr_stat (stat/atx_regrid_stat.hip).  Shared as
// source: the libraries link nothing of each other, so the kernel has internal linkage and each library carries its own copy.
#pragma once

#include <cstdlib>
#include <cstring>

#include "atx_common.hpp"

namespace atx {

// Entries of a table outside [lo, hi), counted on the device: atx_check_indices (lo = 0), and ATX_VALIDATE with a lower bound of -1
// where ATX_ELL_PADDED marks absent entries with -1 and, for ordered traversals, over a row table that must stay inside [0, n_tgt).
static __global__ void __launch_bounds__(kBlock)
check_range_kernel(const int32_t* __restrict__ idx, int64_t n, int64_t lo, int64_t hi, unsigned long long* n_bad) {
    unsigned long long bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const int64_t v = idx[i];
        bad += (v < lo || v >= hi) ? 1u : 0u;
    }
    // wavefront (64-lane) shuffle reduction, then one atomic per wave
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) bad += __shfl_down(bad, off, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0 && bad) atomicAdd(n_bad, bad);
}

// ATX_VALIDATE=1 (read once per process): every gather entry point first range-checks the tables it was handed ON THE DEVICE and
// refuses the launch (ATX_EINVAL, nothing written) if an index points outside the source stack — the kernels trust their tables,
// and an out-of-range read is a GPU fault that can take the whole node with it.  A debugging aid for binders that build their own
// tables: it synchronises the stream and costs a pass over the tables, so it is off by default (the Python mirror validates on the
// host when a plan is built, GatherPlan._check).
static bool validation_on() {
    static const bool on = [] {
        const char* v = std::getenv("ATX_VALIDATE");
        return v && *v && std::strcmp(v, "0") != 0;
    }();
    return on;
}

static int validate_table(const char* fn, const char* what, const int32_t* idx, int64_t n, int64_t lo, int64_t hi, hipStream_t s) {
    if (n <= 0 || !idx) return ATX_OK;
    unsigned long long* n_bad = nullptr;
    int st = hip_status(hipMalloc(reinterpret_cast<void**>(&n_bad), sizeof(unsigned long long)), "ATX_VALIDATE: hipMalloc");
    if (st != ATX_OK) return st;
    unsigned long long host = 0;
    st = hip_status(hipMemsetAsync(n_bad, 0, sizeof(unsigned long long), s), "ATX_VALIDATE: memset");
    if (st == ATX_OK) {
        hipLaunchKernelGGL(check_range_kernel, dim3(grid_for(n, kBlock, kStreamGrid)), dim3(kBlock), 0, s, idx, n, lo, hi, n_bad);
        st = hip_status(hipGetLastError(), "ATX_VALIDATE: launch");
    }
    if (st == ATX_OK) st = hip_status(hipMemcpyAsync(&host, n_bad, sizeof host, hipMemcpyDeviceToHost, s), "ATX_VALIDATE: copy");
    if (st == ATX_OK) st = hip_status(hipStreamSynchronize(s), "ATX_VALIDATE: synchronise");
    (void)hipFree(n_bad);
    if (st != ATX_OK) return st;
    ATX_REQUIRE(host == 0, ATX_EINVAL, "%s: ATX_VALIDATE found %llu entries of %s outside [%lld, %lld) — launch refused", fn, host, what,
                (long long)lo, (long long)hi);
    return ATX_OK;
}

static int check_stack_args(const char* fn, const void* src, const void* out, int64_t n_src, int64_t n_tgt,
                            int64_t n_lev, int64_t sp, int64_t op, int dtype, int layout) {
    ATX_REQUIRE(src && (out || n_tgt == 0), ATX_EINVAL, "%s: null src/out pointer", fn);  // (an output of zero targets may have no storage)
    ATX_REQUIRE(dtype == ATX_F32 || dtype == ATX_F64, ATX_EINVAL, "%s: bad dtype %d", fn, dtype);
    ATX_REQUIRE(layout == ATX_COLUMNS || layout == ATX_FIELDS, ATX_EINVAL, "%s: bad layout %d", fn, layout);
    ATX_REQUIRE(n_src > 0 && n_tgt >= 0 && n_lev > 0, ATX_EINVAL, "%s: bad sizes n_src=%lld n_tgt=%lld n_lev=%lld", fn,
                (long long)n_src, (long long)n_tgt, (long long)n_lev);
    ATX_REQUIRE(n_src <= INT32_MAX && n_tgt <= INT32_MAX && n_lev <= 65535, ATX_ENOTIMPL,
                "%s: sizes exceed int32 indexing (n_src=%lld n_tgt=%lld n_lev=%lld)", fn, (long long)n_src,
                (long long)n_tgt, (long long)n_lev);
    if (layout == ATX_COLUMNS) {
        ATX_REQUIRE(sp >= n_lev && op >= n_lev, ATX_ESHAPE, "%s: column pitch (%lld, %lld) < n_lev %lld", fn,
                    (long long)sp, (long long)op, (long long)n_lev);
    } else {
        ATX_REQUIRE(sp >= n_src && op >= n_tgt, ATX_ESHAPE, "%s: field pitch (%lld, %lld) < points (%lld, %lld)", fn,
                    (long long)sp, (long long)op, (long long)n_src, (long long)n_tgt);
    }
    return ATX_OK;
}

}  // namespace atx
