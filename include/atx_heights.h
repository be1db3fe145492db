/*
 * atx_heights.h — C ABI of libatx_heights, model levels to height levels (MI355X, gfx950): the variables of a model-level column
 * interpolated to geopotential heights above the ground or above mean sea level.  The hydrostatic integral of atx_geopotential.h, the
 * bracket search in geopotential and the interpolation of every variable happen in ONE launch; z itself is never written to memory.
 *
 * A companion library with its own header, as libatx_text, libatx_plan, libatx_mesh, libatx_missing, libatx_stat, libatx_levels and
 * libatx_geopotential are: their entry points, and libatx's (include/atx.h, ATX_VERSION 420), are fixed, tested sets.  The libraries
 * share no symbol and no state; this header includes atx.h for the status codes, atx_dtype and atx_layout, which mean here what they
 * mean there.
 *
 * Conventions (atx.h states them in full; they hold unchanged)
 *  - Plain C types only.  Every pointer named in a signature is a DEVICE pointer (HBM): NO pointer here is a host pointer.  The caller
 *    owns every buffer; the library keeps no state besides a thread-local error string.  A buffer of ZERO elements may be NULL.
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls enqueue work and return without synchronising.
 *  - Return value: ATX_OK (0) or a negative ATX_E* code; atx_heights_last_error() gives the message for the calling thread.
 *  - Every entry point is re-entrant.
 */
#ifndef ATX_HEIGHTS_H
#define ATX_HEIGHTS_H

#include <stddef.h>
#include <stdint.h>

#include "atx.h"

/* Built with -fvisibility=hidden and a version script made from this header: the ATX_HEIGHTS_API declarations below are the library's
 * ONLY dynamic symbols (tests/test_host_api.py checks `nm -D --defined-only` against this header). */
#if defined(_WIN32)
#define ATX_HEIGHTS_API
#else
#define ATX_HEIGHTS_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define ATX_HEIGHTS_VERSION 420 /* goes with ATX_VERSION */

#define ATX_HEIGHTS_MAX_LEVELS 256 /* rows per variable that one call takes (ATX_GEOPOTENTIAL_MAX_LEVELS); more is ATX_ENOTIMPL */

/* ATX_HEIGHTS_VERSION of the library that was loaded. */
ATX_HEIGHTS_API int atx_heights_version(void);

/* The message of the last failed call of the calling thread ("" if none); valid until that thread's next failing call. */
ATX_HEIGHTS_API const char* atx_heights_last_error(void);

/*
 * Model levels to height levels.  For one grid point: the surface pressure sp (Pa), the surface geopotential zs (m^2/s^2), the
 * half-level coefficients A[0..H-1], B[0..H-1] (H = n_half), the n = n_lev rows t[0..n-1] (K), q[0..n-1] (kg/kg) and the n rows
 * x[0..n-1] of each variable, top first.  The rows are the LOWEST n model levels: row k is the 0-based model level j = first + k with
 * first = H - 1 - n, the rule of atx_geopotential_on_model_levels.  A target G is a GEOPOTENTIAL in m^2/s^2 relative to the reference
 * — the caller multiplies metres by g, so the heights are geopotential heights z / g, NOT geometric heights.  All arithmetic is in
 * float64 for both storage widths, one operation at a time, without contraction, with IEEE divisions and the library's own logarithm
 * (<= 1 ulp); the result is rounded once at the store.  Rd = 287.0597, Rv = 461.5250 J / (kg K):
 *     S = 0.0;  z0 = 0.0 (ATX_HEIGHTS_ABOVE_GROUND)  or  zs (ATX_HEIGHTS_ABOVE_SEA)
 *     for k = n - 1 down to 0:          j = first + k            (exactly the terms of atx_geopotential.h)
 *         p_up = A[j] + B[j] * sp       p_dn = A[j + 1] + B[j + 1] * sp
 *         r = Rd * (1.0 - q[k]) + Rv * q[k]
 *         j == 0:  alpha = 0.6931471805599453  (ln 2);  no delta
 *         j  > 0:  delta = log(p_dn / p_up);   alpha = 1.0 - p_up / (p_dn - p_up) * delta
 *         c[k] = z0 + (S + (alpha * r) * t[k])
 *         j  > 0:  S = S + (delta * r) * t[k]
 * For a target G:  n_below = #{k : c[k] < G}, counted over the WHOLE column (a NaN c[k] is not below).
 *     sp != sp or z0 != z0    y = NaN, whatever the policy
 *     n_below == n            (above the top full level)   ATX_HEIGHTS_NEAREST: y = x[0];  ATX_HEIGHTS_MISSING: y = NaN
 *     0 < n_below < n         b = n - n_below, a = b - 1;  w = (c[a] - G) / (c[a] - c[b]);  y = x[a] + w * (x[b] - x[a])
 *     n_below == 0            c[n - 1] != c[n - 1]:  y = NaN
 *                             G >= z0  (between the ground and the lowest full level):  y = x[n - 1]
 *                             otherwise (below the ground)   ATX_HEIGHTS_NEAREST: y = x[n - 1];  ATX_HEIGHTS_MISSING: y = NaN
 * So: c[k] is the unrounded float64 of what atx_geopotential_on_model_levels stores (under ATX_HEIGHTS_ABOVE_SEA a float64 stack's c
 * has that kernel's bits); a target exactly on a full level has w == 0 and returns x[a] (x[a] + 0 * (x[b] - x[a]): its bits for every
 * finite bracket, +0.0 for -0.0); a NaN in t or q at level k makes c NaN at k and above: the targets bracketed by such a level come
 * out NaN, the targets below it are untouched — counting "below" rather than "at or above" is what makes that hold; a NaN in x
 * reaches only the targets whose bracket holds it; n == 1 has no interior.  Which NaN is written is unspecified.  The t / z
 * extrapolations of IFS below the ground are not applied.  earthkit-meteo's hybrid-to-height interpolation is the same family;
 * parity with it is unpinned.
 *
 *   src       n_var variables x n_lev rows each, variables adjacent (rows v * n_lev .. v * n_lev + n_lev - 1 are variable v)
 *   out       n_var x n_tgt rows (row v * n_tgt + i is variable v at targets[i])
 *   t, q      n_lev rows each
 *   All four stacks hold n_pts points in ONE dtype and ONE layout;  src_pitch, t_pitch, q_pitch, out_pitch  per stack, in elements:
 *   between points (ATX_COLUMNS: >= the stack's rows) or between rows (ATX_FIELDS: >= n_pts).
 *   sp        [n_pts], the stacks' type;  zs  [n_pts], the stacks' type: ignored under ATX_HEIGHTS_ABOVE_GROUND (it may be NULL),
 *             required under ATX_HEIGHTS_ABOVE_SEA
 *   A, B      float64 [n_half];  targets  float64 [n_tgt], geopotentials: any order, duplicates allowed, the output is in the given order
 * The bracket and the weight of a (point, target) pair are computed once and applied to all n_var variables.  Both layouts and every
 * load route give the same bits.  ATX_COLUMNS: a workgroup stages the t and q columns of a run of consecutive points in LDS — 16-byte
 * vectors for a stack whose base is 16-byte aligned, whose pitch is a multiple of 16 bytes and whose last vector of a column is inside
 * the pitch (reads may cover the pitch padding inside that vector, nothing beyond), single elements otherwise, decided per stack —
 * computes the terms with one lane per (point, level), sums per point over LDS, finds the brackets with one lane per (point, target),
 * then stages the variables a few at a time through the LDS the terms have left and writes each point's outputs in output order: the
 * LDS of a workgroup does not grow with n_var.  ATX_FIELDS: one lane per (point, target), which walks the column twice.  The padding of
 * out is not written; src, t, q, sp and zs are not modified.
 *
 * Validation comes before anything touches HIP.  ATX_EINVAL: an unknown dtype, layout, reference or policy; n_pts < 0, n_var < 1,
 * n_lev < 1, n_tgt < 0, n_half < 2, n_lev > n_half - 1; a NULL pointer for a buffer that is not empty — zs under
 * ATX_HEIGHTS_ABOVE_SEA among them; out's extent overlapping src's, t's or q's.  ATX_ESHAPE: a pitch too small for the shape.
 * ATX_ENOTIMPL: n_lev > ATX_HEIGHTS_MAX_LEVELS, sizes beyond int32, n_var, n_tgt, n_half, n_var * n_lev or n_var * n_tgt beyond 65535,
 * or (ATX_COLUMNS) one point's columns and brackets beyond the LDS of a workgroup — never a silently wrong result.  No points or no
 * targets: ATX_OK, nothing is launched.
 */
typedef enum { ATX_HEIGHTS_ABOVE_GROUND = 0, ATX_HEIGHTS_ABOVE_SEA = 1 } atx_heights_reference;
typedef enum { ATX_HEIGHTS_NEAREST = 0, ATX_HEIGHTS_MISSING = 1 } atx_heights_outside;
ATX_HEIGHTS_API int atx_heights_interpolate(const void* src, void* out, const void* t, const void* q, const void* sp, const void* zs,
                                            const double* A, const double* B, const double* targets, int64_t n_pts, int64_t n_var,
                                            int64_t n_lev, int64_t n_tgt, int64_t n_half, int64_t src_pitch, int64_t t_pitch,
                                            int64_t q_pitch, int64_t out_pitch, int dtype, int layout, int reference, int outside,
                                            void* stream);

#ifdef __cplusplus
}
#endif

#endif /* ATX_HEIGHTS_H */
