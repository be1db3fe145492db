/*
 * atx_stat.h — C ABI of libatx_stat, the grid-box statistics that go with libatx (MI355X, gfx950): maximum, minimum, mode, variance and
 * standard deviation of the source cells under a target cell, over the rows of a CSR matrix.
 *
 * A companion library with its own header, as libatx_text, libatx_plan, libatx_mesh and libatx_missing are: libatx's entry points
 * are a fixed, tested set (include/atx.h, ATX_VERSION 420).  The libraries share no symbol and no state; this header includes atx.h
 * for the status codes, atx_dtype and atx_layout, which mean here what they mean there.
 *
 * Conventions (atx.h states them in full; they hold unchanged)
 *  - Plain C types only.  Every pointer named in a signature is a DEVICE pointer (HBM).  The caller owns every buffer; the
 *    library keeps no state besides a thread-local error string.  A buffer of ZERO elements may be NULL.
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls enqueue work and return without synchronising.
 *  - Return value: ATX_OK (0) or a negative ATX_E* code; atx_stat_last_error() gives the message for the calling thread.
 *  - Every entry point is re-entrant.
 */
#ifndef ATX_STAT_H
#define ATX_STAT_H

#include <stddef.h>
#include <stdint.h>

#include "atx.h"

/* Built with -fvisibility=hidden and a version script made from this header: the ATX_STAT_API declarations below are the
 * library's ONLY dynamic symbols (tests/test_host_api.py checks `nm -D --defined-only` against this header). */
#if defined(_WIN32)
#define ATX_STAT_API
#else
#define ATX_STAT_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define ATX_STAT_VERSION 420 /* goes with ATX_VERSION */

/* ATX_STAT_VERSION of the library that was loaded. */
ATX_STAT_API int atx_stat_version(void);

/* The message of the last failed call of the calling thread ("" if none); valid until that thread's next failing call. */
ATX_STAT_API const char* atx_stat_last_error(void);

/*
 * atx_regrid_csr (atx.h) with a reduction other than the weighted sum: row t of the matrix names the source cells under target t
 * and their shares (interp.box_average_rows builds such rows; any CSR is taken as the definition of the cells).  For one output
 * element (target t, level l) in the stack's type T, every operation rounded on its own (no fused multiply-add), the entries j of
 * row t (indptr[t] .. indptr[t+1]-1) in table order:
 *     w_j = data[j], or T(1) where data == NULL
 *     jh  = the first entry of the row with the largest w (strict >)
 *     for every entry:  tot = tot + w_j;  x_j = src[indices[j], l]
 *         x_j != x_j : missing = true;  j == jh: heaviest_missing = true
 *         else       : j is VALID;  den = den + w_j
 *     out = NaN  when the row has no valid entry (an empty row included)
 *         = NaN  under ATX_STAT_MISSING_ANY when missing;  under ATX_STAT_MISSING_HEAVIEST when heaviest_missing
 *         = NaN  when den < T(min_valid) * tot
 *     otherwise, over the valid entries in row order:
 *       MAXIMUM   m = first valid x;  then  m = (x_j > m) ? x_j : m
 *       MINIMUM   the same with <
 *       MODE      W_j = sum from T(0), in row order, of w_i over valid i with x_i == x_j
 *                 best = first valid j;  a later j replaces it when  W_j > W_best,  or  W_j == W_best and x_j < x_best
 *                 out = x_best
 *       VARIANCE  num = sum of (w_j * x_j);  mean = num / den;  d_j = x_j - mean;  s = sum of (w_j * (d_j * d_j));  out = s / den
 *       STDDEV    sqrt(VARIANCE), correctly rounded
 * (tot, den, num, s and every W start at T(0); the divisions are IEEE divisions.)
 * So: +-inf are values, and VARIANCE over them is whatever the arithmetic gives; -0.0 == 0.0 are one class and one extreme, and the
 * first one met is written; an equal-weight tie in MODE goes to the smaller value; a NaN under a zero weight still counts as
 * missing; a negative sum of valid weights gives NaN even with min_valid = 0.  Which NaN is written is unspecified.  Where every
 * weight is finite and non-negative, MAXIMUM and MINIMUM under ANY or ALL with min_valid = 0 do not depend on the weights: a caller
 * that knows so may pass data = NULL and gets the same bits with fewer table bytes read.
 * MIR's grid-box-statistics is the same family; parity with MIR is unpinned: the tie rule and the missing-value policies are this
 * project's.
 *   statistic: atx_statistic; policy: atx_stat_missing; min_valid in [0, 1]: the share of the row's weight that must be valid.
 * Arguments, validation (ATX_VALIDATE=1 in the environment range-checks the tables on the device first and synchronises) and status
 * codes are those of atx_regrid_csr; in addition an unknown statistic or policy, a min_valid outside [0, 1] (or NaN) and data == NULL
 * with MODE, VARIANCE or STDDEV are ATX_EINVAL.  ATX_COLUMNS only: ATX_FIELDS is ATX_ENOTIMPL (convert with atx_relayout).  No level
 * program, no target mask, natural target order.  16-byte aligned bases with pitches that are multiples of 16 bytes take 16-byte
 * vectors (writes may cover the pitch padding inside the last vector of a column, nothing beyond), anything else single elements.
 * MODE keeps a bounded table of classes per element and walks the row once; a row with more distinct values than the table holds
 * is redone by the quadratic walk of the statement (same bits, the time of a row length squared).
 */
typedef enum { ATX_STAT_MAXIMUM = 0, ATX_STAT_MINIMUM = 1, ATX_STAT_MODE = 2, ATX_STAT_VARIANCE = 3, ATX_STAT_STDDEV = 4 } atx_statistic;
typedef enum { ATX_STAT_MISSING_ANY = 0, ATX_STAT_MISSING_ALL = 1, ATX_STAT_MISSING_HEAVIEST = 2 } atx_stat_missing;
ATX_STAT_API int atx_regrid_csr_stat(const void* src, void* out, const int32_t* indptr, const int32_t* indices, const void* data,
                                     int64_t n_src, int64_t n_tgt, int64_t nnz, int64_t n_lev, int64_t src_pitch, int64_t out_pitch,
                                     int dtype, int layout, int statistic, int policy, double min_valid, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* ATX_STAT_H */
