// The C ABI of the gather: atx_regrid_ell / _batch / _ordered, atx_regrid_csr / _ordered, atx_check_indices, atx_set_tuning.
//
// Replaces, for all levels of a stack in ONE launch, the per-field statements
//   R: filters/fields/regrid.py:380  data[..., self.nearest_grid_points]
//   R: filters/fields/regrid.py:310  self.matrix @ data          (scipy csr_matvec)
//   R: filters/fields/regrid.py:420  data[..., self.mask]
// that the reference runs once per 2-D field in a Python loop (regrid.py:204-208).
//
// This file checks the arguments (the stack check and the ATX_VALIDATE range check are atx_regrid_check.hpp's), cuts a batch into
// launches of kMaxBatch stacks and falls back to gather-then-program when a fused program does not fit in LDS.  The kernels (HBM-bound gathers, no MFMA; DESIGN.md
// §3) are in atx_regrid_columns.inc and atx_regrid_fields.inc, instantiated per element type in atx_regrid_f32.hip /
// atx_regrid_f64.hip and reached through regrid_ell_typed<T> / regrid_csr_typed<T> (atx_regrid_decl.hpp).
#include <type_traits>

#include "atx_common.hpp"
#include "atx_regrid_check.hpp"
#include "atx_regrid_decl.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace atx {

thread_local int g_tile_override = 0;  // tuning hook (atx_set_tuning): per calling thread, meant for benchmarks and tests (results never depend on it)

// The launch form of this thread's last gather (atx_last_gather_route): filled by the launchers, a second cell beside g_last_route.
__thread GatherRoute g_gather_route = {nullptr, nullptr, nullptr, nullptr, 0, false, false, false, false, false};

}  // namespace atx

using namespace atx;

extern "C" const char* atx_last_gather_route(void) {
    static thread_local char text[128];
    const GatherRoute& r = g_gather_route;
    if (!r.table) return "none";
    std::snprintf(text, sizeof text, "%s/%s/%s/%s/k%d/%s/%s/%s/%s", r.table, r.kernel, r.split ? "split" : r.epilogue, r.width, r.k,
                  r.padded ? "padded" : "plain", r.weighted ? "weighted" : "pure", r.stripe ? "stripe" : "range", r.ordered ? "ordered" : "natural");
    return text;
}

extern "C" int atx_set_tuning(int tile) {
    g_tile_override = tile;
    return ATX_OK;
}

static int regrid_ell_common(const char* fn, const void* const* srcs, void* const* outs, int32_t n_stack, const int32_t* idx,
                             const void* w, int64_t n_src, int64_t n_tgt, int32_t k, int64_t n_lev, int64_t src_pitch,
                             int64_t out_pitch, int dtype, int layout, int32_t flags, const atx_level_op* prog,
                             const atx_level_op* vec_prog, const atx_level_op* host_prog, int32_t n_stage, const uint8_t* tgt_mask,
                             const int32_t* tgt_rows, void* stream) {
    g_gather_route.table = nullptr;  // "none" until a gather launches (atx_last_gather_route)
    ATX_REQUIRE(srcs && outs && n_stack >= 1, ATX_EINVAL, "%s: needs at least one stack", fn);
    ATX_REQUIRE(!tgt_rows || layout == ATX_COLUMNS, ATX_ENOTIMPL, "%s: an ordered traversal (tgt_rows) is available for ATX_COLUMNS stacks only", fn);
    for (int32_t i = 0; i < n_stack; ++i) {
        int st = check_stack_args(fn, srcs[i], outs[i], n_src, n_tgt, n_lev, src_pitch, out_pitch, dtype, layout);
        if (st != ATX_OK) return st;
    }
    ATX_REQUIRE(idx || n_tgt == 0, ATX_EINVAL, "%s: null idx", fn);
    ATX_REQUIRE(k >= 1 && k <= 64, ATX_EINVAL, "%s: k=%d outside [1, 64]", fn, k);
    ATX_REQUIRE(w || k == 1, ATX_EINVAL, "%s: a pure gather (w == NULL) needs k == 1, got %d", fn, k);
    ATX_REQUIRE((flags & ~ATX_ELL_PADDED) == 0, ATX_EINVAL, "%s: unknown flags 0x%x", fn, flags);
    ATX_REQUIRE(!(flags & ATX_ELL_PADDED) || w, ATX_EINVAL, "%s: ATX_ELL_PADDED needs weights", fn);
    const bool pad = (flags & ATX_ELL_PADDED) != 0;
    ATX_REQUIRE((prog == nullptr) == (n_stage == 0) && n_stage >= 0 && n_stage <= 8, ATX_EINVAL,
                "%s: prog/n_stage mismatch (n_stage=%d)", fn, n_stage);
    ATX_REQUIRE(prog || (!vec_prog && !host_prog), ATX_EINVAL, "%s: vec_prog / host_prog accompany prog, which is NULL", fn);
    if (n_tgt == 0) return ATX_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (validation_on()) {
        int st = validate_table(fn, "idx", idx, n_tgt * k, pad ? -1 : 0, n_src, s);
        if (st == ATX_OK && tgt_rows) st = validate_table(fn, "tgt_rows", tgt_rows, n_tgt, 0, n_tgt, s);
        if (st != ATX_OK) return st;
    }
    Epilogue epi;
    epi.prog = prog;
    epi.vec_prog = vec_prog;
    epi.host_prog = host_prog;
    epi.n_stage = n_stage;
    epi.mask = tgt_mask;
    epi.tgt_rows = tgt_rows;
    for (int32_t first = 0; first < n_stack; first += kMaxBatch) {
        EllBatch batch;
        batch.n = n_stack - first < kMaxBatch ? n_stack - first : kMaxBatch;
        for (int i = 0; i < kMaxBatch; ++i) {
            batch.src[i] = i < batch.n ? srcs[first + i] : nullptr;
            batch.out[i] = i < batch.n ? outs[first + i] : nullptr;
        }
        auto run = [&](const Epilogue& e) {
            if (dtype == ATX_F32) return regrid_ell_typed<float>(batch, idx, w, n_tgt, k, (int)n_lev, src_pitch, out_pitch, layout, pad, e, s);
            return regrid_ell_typed<double>(batch, idx, w, n_tgt, k, (int)n_lev, src_pitch, out_pitch, layout, pad, e, s);
        };
        int rc = run(epi);
        if (rc == ATX_SPLIT_PROGRAM) {  // the fused tables do not fit in LDS: the plain gather, then the program on its output in place
            Epilogue plain;
            plain.tgt_rows = tgt_rows;
            rc = run(plain);
            g_gather_route.split = true;
            for (int i = 0; i < batch.n && rc == ATX_OK; ++i)
                rc = atx_pointwise_stack(batch.out[i], batch.out[i], n_tgt, n_lev, out_pitch, out_pitch, dtype, layout, prog, vec_prog, host_prog,
                                         n_stage, tgt_mask, stream);
        }
        if (rc != ATX_OK) return rc;
    }
    return ATX_OK;
}

extern "C" int atx_regrid_ell(const void* src, void* out, const int32_t* idx, const void* w, int64_t n_src,
                              int64_t n_tgt, int32_t k, int64_t n_lev, int64_t src_pitch, int64_t out_pitch,
                              int dtype, int layout, int32_t flags, const atx_level_op* prog, const atx_level_op* vec_prog,
                              const atx_level_op* host_prog, int32_t n_stage, const uint8_t* tgt_mask, void* stream) {
    return regrid_ell_common("atx_regrid_ell", &src, &out, 1, idx, w, n_src, n_tgt, k, n_lev, src_pitch, out_pitch, dtype,
                             layout, flags, prog, vec_prog, host_prog, n_stage, tgt_mask, nullptr, stream);
}

extern "C" int atx_regrid_ell_batch(const void* const* srcs, void* const* outs, int32_t n_stack, const int32_t* idx,
                                    const void* w, int64_t n_src, int64_t n_tgt, int32_t k, int64_t n_lev,
                                    int64_t src_pitch, int64_t out_pitch, int dtype, int layout, int32_t flags,
                                    const atx_level_op* prog, const atx_level_op* vec_prog, const atx_level_op* host_prog,
                                    int32_t n_stage, const uint8_t* tgt_mask, void* stream) {
    return regrid_ell_common("atx_regrid_ell_batch", srcs, outs, n_stack, idx, w, n_src, n_tgt, k, n_lev, src_pitch, out_pitch,
                             dtype, layout, flags, prog, vec_prog, host_prog, n_stage, tgt_mask, nullptr, stream);
}

extern "C" int atx_regrid_ell_ordered(const void* const* srcs, void* const* outs, int32_t n_stack, const int32_t* idx,
                                      const void* w, const int32_t* tgt_rows, int64_t n_src, int64_t n_tgt, int32_t k, int64_t n_lev,
                                      int64_t src_pitch, int64_t out_pitch, int dtype, int layout, int32_t flags,
                                      const atx_level_op* prog, const atx_level_op* vec_prog, const atx_level_op* host_prog,
                                      int32_t n_stage, const uint8_t* tgt_mask, void* stream) {
    ATX_REQUIRE(tgt_rows, ATX_EINVAL, "atx_regrid_ell_ordered: null tgt_rows (use atx_regrid_ell_batch for the natural order)");
    return regrid_ell_common("atx_regrid_ell_ordered", srcs, outs, n_stack, idx, w, n_src, n_tgt, k, n_lev, src_pitch, out_pitch,
                             dtype, layout, flags, prog, vec_prog, host_prog, n_stage, tgt_mask, tgt_rows, stream);
}

static int regrid_csr_common(const char* fn, const void* src, void* out, const int32_t* indptr, const int32_t* indices,
                             const void* data, int64_t n_src, int64_t n_tgt, int64_t nnz, int64_t n_lev,
                             int64_t src_pitch, int64_t out_pitch, int dtype, int layout, const atx_level_op* prog,
                             int32_t n_stage, const uint8_t* tgt_mask, const int32_t* tgt_rows, void* stream) {
    g_gather_route.table = nullptr;  // "none" until a gather launches (atx_last_gather_route)
    int st = check_stack_args(fn, src, out, n_src, n_tgt, n_lev, src_pitch, out_pitch, dtype, layout);
    if (st != ATX_OK) return st;
    ATX_REQUIRE(indptr || n_tgt == 0, ATX_EINVAL, "%s: null indptr", fn);
    ATX_REQUIRE(nnz >= 0 && nnz <= INT32_MAX, ATX_ENOTIMPL, "%s: nnz=%lld outside int32", fn, (long long)nnz);
    ATX_REQUIRE(nnz == 0 || (indices && data), ATX_EINVAL, "%s: null indices/data", fn);
    ATX_REQUIRE((prog == nullptr) == (n_stage == 0) && n_stage >= 0 && n_stage <= 8, ATX_EINVAL,
                "%s: prog/n_stage mismatch (n_stage=%d)", fn, n_stage);
    if (n_tgt == 0) return ATX_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (validation_on()) {
        int st = validate_table(fn, "indices", indices, nnz, 0, n_src, s);
        if (st == ATX_OK) st = validate_table(fn, "indptr", indptr, n_tgt + 1, 0, nnz + 1, s);
        if (st == ATX_OK && tgt_rows) st = validate_table(fn, "tgt_rows", tgt_rows, n_tgt, 0, n_tgt, s);
        if (st != ATX_OK) return st;
    }
    auto run = [&](const atx_level_op* p, int32_t stages, const uint8_t* m) {
        if (dtype == ATX_F32)
            return regrid_csr_typed<float>(src, out, indptr, indices, data, n_tgt, nnz, (int)n_lev, src_pitch, out_pitch, layout, p, stages, m, tgt_rows, s);
        return regrid_csr_typed<double>(src, out, indptr, indices, data, n_tgt, nnz, (int)n_lev, src_pitch, out_pitch, layout, p, stages, m, tgt_rows, s);
    };
    int rc = run(prog, n_stage, tgt_mask);
    if (rc == ATX_SPLIT_PROGRAM) {  // the fused tables do not fit in LDS: the plain product, then the program on its output in place
        rc = run(nullptr, 0, nullptr);
        g_gather_route.split = true;
        if (rc == ATX_OK)
            rc = atx_pointwise_stack(out, out, n_tgt, n_lev, out_pitch, out_pitch, dtype, layout, prog, nullptr, nullptr, n_stage, tgt_mask, stream);
    }
    return rc;
}

extern "C" int atx_regrid_csr(const void* src, void* out, const int32_t* indptr, const int32_t* indices,
                              const void* data, int64_t n_src, int64_t n_tgt, int64_t nnz, int64_t n_lev,
                              int64_t src_pitch, int64_t out_pitch, int dtype, int layout, const atx_level_op* prog,
                              int32_t n_stage, const uint8_t* tgt_mask, void* stream) {
    return regrid_csr_common("atx_regrid_csr", src, out, indptr, indices, data, n_src, n_tgt, nnz, n_lev, src_pitch, out_pitch, dtype, layout,
                             prog, n_stage, tgt_mask, nullptr, stream);
}

extern "C" int atx_regrid_csr_ordered(const void* src, void* out, const int32_t* indptr, const int32_t* indices,
                                      const void* data, const int32_t* tgt_rows, int64_t n_src, int64_t n_tgt, int64_t nnz, int64_t n_lev,
                                      int64_t src_pitch, int64_t out_pitch, int dtype, int layout, const atx_level_op* prog,
                                      int32_t n_stage, const uint8_t* tgt_mask, void* stream) {
    ATX_REQUIRE(tgt_rows, ATX_EINVAL, "atx_regrid_csr_ordered: null tgt_rows (use atx_regrid_csr for the natural order)");
    return regrid_csr_common("atx_regrid_csr_ordered", src, out, indptr, indices, data, n_src, n_tgt, nnz, n_lev, src_pitch, out_pitch, dtype,
                             layout, prog, n_stage, tgt_mask, tgt_rows, stream);
}

extern "C" int atx_check_indices(const int32_t* idx, int64_t n, int64_t n_src, int64_t* n_bad, void* stream) {
    ATX_REQUIRE(n_bad && (idx || n == 0), ATX_EINVAL, "atx_check_indices: null pointer");
    ATX_REQUIRE(n >= 0 && n_src >= 0, ATX_EINVAL, "atx_check_indices: negative size");
    hipStream_t s = static_cast<hipStream_t>(stream);
    int st = hip_status(hipMemsetAsync(n_bad, 0, sizeof(int64_t), s), "atx_check_indices memset");
    if (st != ATX_OK) return st;
    if (n == 0) return ATX_OK;
    hipLaunchKernelGGL(check_range_kernel, dim3(grid_for(n, kBlock, kStreamGrid)), dim3(kBlock), 0, s, idx, n, (int64_t)0, n_src,
                       reinterpret_cast<unsigned long long*>(n_bad));
    ATX_LAUNCH_CHECK("check_indices");
    return ATX_OK;
}
