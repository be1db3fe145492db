/*
 * atx_geopotential.h — C ABI of libatx_geopotential, the hydrostatic integral that goes with libatx and libatx_levels (MI355X,
 * gfx950): the geopotential on model levels from temperature, humidity, surface pressure and surface geopotential, one column at a time.
 *
 * A companion library with its own header, as libatx_text, libatx_plan, libatx_mesh, libatx_missing, libatx_stat and libatx_levels
 * are: their entry points, and libatx's (include/atx.h, ATX_VERSION 420), are fixed, tested sets.  The libraries share no symbol and
 * no state; this header includes atx.h for the status codes, atx_dtype and atx_layout, which mean here what they mean there.
 *
 * Conventions (atx.h states them in full; they hold unchanged)
 *  - Plain C types only.  Every pointer named in a signature is a DEVICE pointer (HBM): NO pointer here is a host pointer.  The caller
 *    owns every buffer; the library keeps no state besides a thread-local error string.  A buffer of ZERO elements may be NULL.
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls enqueue work and return without synchronising.
 *  - Return value: ATX_OK (0) or a negative ATX_E* code; atx_geopotential_last_error() gives the message for the calling thread.
 *  - Every entry point is re-entrant.
 */
#ifndef ATX_GEOPOTENTIAL_H
#define ATX_GEOPOTENTIAL_H

#include <stddef.h>
#include <stdint.h>

#include "atx.h"

/* Built with -fvisibility=hidden and a version script made from this header: the ATX_GEOPOTENTIAL_API declarations below are the
 * library's ONLY dynamic symbols (tests/test_host_api.py checks `nm -D --defined-only` against this header). */
#if defined(_WIN32)
#define ATX_GEOPOTENTIAL_API
#else
#define ATX_GEOPOTENTIAL_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define ATX_GEOPOTENTIAL_VERSION 420 /* goes with ATX_VERSION */

#define ATX_GEOPOTENTIAL_MAX_LEVELS 256 /* rows that one call takes (ATX_LEVELS_MAX_LEVELS of atx_levels.h); more is ATX_ENOTIMPL */

/* ATX_GEOPOTENTIAL_VERSION of the library that was loaded. */
ATX_GEOPOTENTIAL_API int atx_geopotential_version(void);

/* The message of the last failed call of the calling thread ("" if none); valid until that thread's next failing call. */
ATX_GEOPOTENTIAL_API const char* atx_geopotential_last_error(void);

/*
 * Geopotential on model levels: the hydrostatic integral from the ground, which IFS does not archive and atx_levels_interpolate
 * (atx_levels.h) needs for z500 and the rest.  For one grid point: the surface pressure sp (Pa), the surface geopotential zs
 * (m^2/s^2), the half-level coefficients A[0..H-1], B[0..H-1] (H = n_half) and the n = n_lev rows t[0..n-1] (K), q[0..n-1] (kg/kg),
 * top first.  The rows are the LOWEST n model levels: row k is the 0-based model level j = first + k with first = H - 1 - n, so row
 * n - 1 always sits on the ground half level and a subset such as levels 60-137 works.  All arithmetic is in float64 for both
 * storage widths, one operation at a time, without contraction, with IEEE divisions and the library's own logarithm (<= 1 ulp); the
 * result is rounded once at the store.  Rd = 287.0597, Rv = 461.5250 J / (kg K):
 *     S = 0.0
 *     for k = n - 1 down to 0:          j = first + k
 *         p_up = A[j] + B[j] * sp       p_dn = A[j + 1] + B[j + 1] * sp
 *         r = Rd * (1.0 - q[k]) + Rv * q[k]
 *         j == 0:  alpha = 0.6931471805599453  (ln 2, the IFS top level);  no delta
 *         j  > 0:  delta = log(p_dn / p_up);   alpha = 1.0 - p_up / (p_dn - p_up) * delta
 *         z[k] = zs + (S + (alpha * r) * t[k])
 *         j  > 0:  S = S + (delta * r) * t[k]
 * This is the IFS discretisation as ECMWF's compute-geopotential-on-model-levels script writes it — delta for the full layers below a
 * level, alpha for the level's own half layer — with this library's moist gas constant r t in the place of Rd Tv.  (The dphi of
 * atx_pressure_at_height_stack, atx.h, sums alpha r t over the layers below, earthkit-meteo's reading: the same value for the lowest
 * level only.)  So: the sum runs sequentially from the ground; a NaN in t[k] or q[k] reaches z[k] and every level above it, nothing
 * below it; a NaN sp makes every level NaN whose alpha or S holds a pressure — the whole column, a column that is model level 0 alone
 * aside; a table with p_up == 0 at j > 0 gives what IEEE gives (delta = +inf, alpha = 1 - 0 * inf = NaN); which NaN is written is
 * unspecified; with zs == NULL the bottom row is (alpha * r) * t of that level exactly (-0.0 comes out as +0.0).  Parity with
 * earthkit-meteo and MARS is unpinned.
 *
 *   t, q, out   n_lev rows each, n_pts points, ONE dtype and ONE layout for the three;  t_pitch, q_pitch, out_pitch  per stack, in
 *               elements: between points (ATX_COLUMNS: >= n_lev) or between rows (ATX_FIELDS: >= n_pts)
 *   sp          [n_pts], the stacks' type;  zs  [n_pts], the stacks' type, or NULL: 0.0 everywhere;  A, B  float64 [n_half]
 * Both layouts and both load routes give the same bits.  ATX_COLUMNS: a workgroup stages the t and q columns of a run of consecutive
 * points in LDS with loads that cover each run contiguously — 16-byte vectors for a stack whose base is 16-byte aligned, whose pitch
 * is a multiple of 16 bytes and whose last vector of a column is inside the pitch (reads may cover the pitch padding inside that
 * vector, nothing beyond), single elements otherwise, decided for t and q independently — computes the terms with one lane per
 * (point, level), sums per point over LDS and writes each point's n_lev values as one contiguous run.  ATX_FIELDS: one lane per point,
 * bottom-up.  The padding of out is not written; t, q, sp and zs are not modified.
 *
 * Validation comes before anything touches HIP.  ATX_EINVAL: an unknown dtype or layout; n_pts < 0, n_lev < 1, n_half < 2,
 * n_lev > n_half - 1; a NULL t, q, sp, out, A or B of a call that is not empty; out's extent overlapping t's or q's.  ATX_ESHAPE: a
 * pitch too small for the shape.  ATX_ENOTIMPL: n_lev > ATX_GEOPOTENTIAL_MAX_LEVELS, sizes beyond int32.  No points: ATX_OK, nothing
 * is launched.
 */
ATX_GEOPOTENTIAL_API int atx_geopotential_on_model_levels(const void* t, const void* q, const void* sp, const void* zs, const double* A,
                                                          const double* B, void* out, int64_t n_pts, int64_t n_lev, int64_t n_half,
                                                          int64_t t_pitch, int64_t q_pitch, int64_t out_pitch, int dtype, int layout,
                                                          void* stream);

#ifdef __cplusplus
}
#endif

#endif /* ATX_GEOPOTENTIAL_H */
