/*
 * atx_plan.h — C ABI of libatx_plan, the plan-time kernels that go with libatx (MI355X, gfx950).
 *
 * A companion library with its own header, as libatx_text is: libatx's entry points are a
 * fixed set (include/atx.h, ATX_VERSION 420) that APPLY a regrid operator; this library
 * BUILDS one in HBM.  The libraries share no symbol and no state; this header includes
 * atx.h only for the status codes (ATX_OK, ATX_EINVAL, ATX_EHIP, ...), which mean here
 * what they mean there.
 *
 * Conventions (atx.h states them in full; they hold unchanged)
 *  - Plain C types only.  Every pointer named in a signature is a DEVICE pointer
 *    (HBM).  The caller owns every buffer; the library allocates nothing and
 *    keeps no state besides a thread-local error string.  A buffer of ZERO
 *    elements may be NULL: the call validates the rest, launches nothing and
 *    returns ATX_OK.
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls
 *    enqueue work and return without synchronising.
 *  - Return value: ATX_OK (0) or a negative ATX_E* code; atx_plan_last_error()
 *    gives the message for the calling thread.  Nothing throws across the ABI.
 *  - Every entry point is re-entrant.
 *
 * A *row table* describes a row-structured global grid of R rows of constant latitude, north to south, row r holding len[r] >= 2
 * equally spaced longitudes from 0, points in row-major order:
 *   z      double [R + 1]  sine of the latitude EDGES of the rows, strictly descending, z[0] = 1, z[R] = -1 (computed by the caller)
 *   len    int64  [R]      points per row
 *   start  int64  [R + 1]  index of the first point of each row; start[R] is the number of points
 * The caller validates the CONTENT of the tables before upload (the library cannot read HBM on the host); the library checks sizes
 * and pointers, and its kernels never index outside the arrays as sized here whatever the tables hold.
 */
#ifndef ATX_PLAN_H
#define ATX_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include "atx.h"

/* Built with -fvisibility=hidden and a version script made from this header: the ATX_PLAN_API declarations below are the library's
 * ONLY dynamic symbols (tests/test_box_average_host.py checks `nm -D --defined-only` against this header). */
#if defined(_WIN32)
#define ATX_PLAN_API
#else
#define ATX_PLAN_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define ATX_PLAN_VERSION 420 /* goes with ATX_VERSION */

/* ATX_PLAN_VERSION of the library that was loaded. */
ATX_PLAN_API int atx_plan_version(void);

/* The message of the last failed call of the calling thread ("" if none); valid until that thread's next failing call. */
ATX_PLAN_API const char* atx_plan_last_error(void);

/*
 * Grid-box-average weights between two row-structured grids (interp.box_average_rows states them; no reference counterpart:
 * the reference hands the method to earthkit-regrid).  One target cell per lane.
 *
 *   latitude   target row r and source row q overlap by dz = min(zt[r], zs[q]) - max(zt[r+1], zs[q+1]); q takes part iff
 *              dz > 2^-40 * (zt[r] - zt[r+1]).
 *   longitude  cell i of nt and cell j of ns overlap by ov units of 360 / (2 ns nt) degrees, an exact integer; the entry exists
 *              iff ov > 0.  The cells of one source row that a target cell meets are a cyclic run.
 *   weights    raw = dz * ((double)ov / (double)(2 ns nt)); the entries of a target are kept in ascending source index,
 *              tot is their sum from 0 in that order, w = raw / tot.
 *
 * atx_plan_box_average_count writes count[t], the number of entries of target t, for t in [0, n_tgt).  The caller scans the counts
 * into indptr (int32 [n_tgt + 1], indptr[0] = 0, indptr[n_tgt] = nnz) and atx_plan_box_average_fill writes
 * indices[indptr[t] .. indptr[t+1]) and data[...] likewise; an entry that would fall outside [indptr[t], min(indptr[t+1], nnz)) is
 * not written.
 *
 * ATX_EINVAL: n_src_rows or n_tgt_rows outside 1 .. 2^31 - 1, n_src outside 1 .. 2^31 - 1, n_tgt < 0, nnz outside 0 .. 2^31 - 1,
 * or a NULL pointer with n_tgt > 0 — nothing is launched.  n_tgt == 0: ATX_OK, nothing launched, the pointers may be NULL.
 */
ATX_PLAN_API int atx_plan_box_average_count(const double* zs, const int64_t* src_len, const int64_t* src_start, int64_t n_src_rows,
                                            int64_t n_src, const double* zt, const int64_t* tgt_len, const int64_t* tgt_start,
                                            int64_t n_tgt_rows, int64_t n_tgt, int64_t* count, void* stream);

ATX_PLAN_API int atx_plan_box_average_fill(const double* zs, const int64_t* src_len, const int64_t* src_start, int64_t n_src_rows,
                                           int64_t n_src, const double* zt, const int64_t* tgt_len, const int64_t* tgt_start,
                                           int64_t n_tgt_rows, int64_t n_tgt, const int32_t* indptr, int64_t nnz, int32_t* indices,
                                           double* data, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* ATX_PLAN_H */
