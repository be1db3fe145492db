/*
 * atx_missing.h — C ABI of libatx_missing, the weighted gather with missing values that goes with libatx (MI355X, gfx950).
 *
 * A companion library with its own header, as libatx_text, libatx_plan and libatx_mesh are: libatx's entry points are a
 * fixed, tested set (include/atx.h, ATX_VERSION 420).  The libraries share no symbol and no state; this header includes
 * atx.h for the status codes, atx_dtype, atx_layout and ATX_ELL_PADDED, which mean here what they mean there.
 *
 * Conventions (atx.h states them in full; they hold unchanged)
 *  - Plain C types only.  Every pointer named in a signature is a DEVICE pointer (HBM).  The caller owns every buffer; the
 *    library keeps no state besides a thread-local error string.  A buffer of ZERO elements may be NULL.
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls enqueue work and return without synchronising.
 *  - Return value: ATX_OK (0) or a negative ATX_E* code; atx_missing_last_error() gives the message for the calling thread.
 *  - Every entry point is re-entrant.
 */
#ifndef ATX_MISSING_H
#define ATX_MISSING_H

#include <stddef.h>
#include <stdint.h>

#include "atx.h"

/* Built with -fvisibility=hidden and a version script made from this header: the ATX_MISSING_API declarations below are the
 * library's ONLY dynamic symbols (tests/test_regrid_missing_host.py checks `nm -D --defined-only` against this header). */
#if defined(_WIN32)
#define ATX_MISSING_API
#else
#define ATX_MISSING_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define ATX_MISSING_VERSION 420 /* goes with ATX_VERSION */

/* ATX_MISSING_VERSION of the library that was loaded. */
ATX_MISSING_API int atx_missing_version(void);

/* The message of the last failed call of the calling thread ("" if none); valid until that thread's next failing call. */
ATX_MISSING_API const char* atx_missing_last_error(void);

/*
 * atx_regrid_ell / atx_regrid_csr (atx.h) for stacks with MISSING VALUES: a NaN source is dropped, the remaining weights
 * renormalise, and a policy decides when the target itself is missing.  For one output element (target t, level l) in the stack's
 * type T, every operation rounded on its own (no fused multiply-add), the entries j of row t in table order (ELL: j = 0 .. k-1, a
 * negative index is an absent entry and skipped; CSR: indptr[t] .. indptr[t+1]-1):
 *     jh  = the first present entry of the row with the largest weight (strict >); none in a row without present entries
 *     x = src[idx_j, l];  tot = tot + w_j
 *     x != x :  missing = true;  j == jh: heaviest_missing = true
 *     else   :  num = num + (w_j * x);  den = den + w_j;  n_valid += 1
 *     out = num                        when nothing was missing — scipy's csr_matvec bit for bit, no division
 *         = NaN                        when n_valid == 0
 *         = NaN                        under ATX_MISSING_HEAVIEST when heaviest_missing
 *         = NaN                        when den < T(min_valid) * tot
 *         = num / den                  otherwise (IEEE division)
 * So: +-inf sources are values; a NaN under a zero weight is dropped (the plain gather gives NaN there); a negative or zero sum of
 * valid weights gives NaN; a row without present entries gives 0 as the plain gather does.  Which NaN is written is unspecified.
 * The policy names are MIR's (missing-if-all-missing, missing-if-heaviest-missing); parity with MIR is unpinned.
 *   policy: atx_missing_policy; min_valid in [0, 1]: the share of the row's weight that must be valid.
 *   flags: 0 or ATX_ELL_PADDED, as atx_regrid_ell declares them (a negative index is skipped either way).
 * Arguments, validation (ATX_VALIDATE=1 in the environment range-checks the tables on the device first and synchronises) and status
 * codes are those of atx_regrid_ell / atx_regrid_csr; in addition w == NULL, an unknown policy and a min_valid outside [0, 1] (or
 * NaN) are ATX_EINVAL.  ATX_COLUMNS only: ATX_FIELDS is ATX_ENOTIMPL (convert with atx_relayout).  No level program, no target
 * mask, natural target order.  16-byte aligned bases with pitches that are multiples of 16 bytes take 16-byte vectors (writes may
 * cover the pitch padding inside the last vector of a column, nothing beyond), anything else single elements.
 */
typedef enum { ATX_MISSING_ALL = 0, ATX_MISSING_HEAVIEST = 1 } atx_missing_policy;
ATX_MISSING_API int atx_regrid_ell_missing(const void* src, void* out, const int32_t* idx, const void* w, int64_t n_src, int64_t n_tgt,
                                           int32_t k, int64_t n_lev, int64_t src_pitch, int64_t out_pitch, int dtype, int layout,
                                           int32_t flags, int policy, double min_valid, void* stream);
ATX_MISSING_API int atx_regrid_csr_missing(const void* src, void* out, const int32_t* indptr, const int32_t* indices, const void* data,
                                           int64_t n_src, int64_t n_tgt, int64_t nnz, int64_t n_lev, int64_t src_pitch, int64_t out_pitch,
                                           int dtype, int layout, int policy, double min_valid, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* ATX_MISSING_H */
