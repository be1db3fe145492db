/*
 * atx_pltz.h — C ABI of libatx_pltz, temperature and geopotential on pressure levels with the IFS extrapolations under the ground, and
 * mean sea level pressure (MI355X, gfx950).  The hydrostatic integral of atx_geopotential.h, the bracket search in pressure, the
 * interpolation of t and of z, the extrapolations and msl happen in ONE launch; z on model levels is never written to memory.
 *
 * A companion library with its own header, as libatx_text, libatx_plan, libatx_mesh, libatx_missing, libatx_stat, libatx_levels,
 * libatx_geopotential and libatx_heights are: their entry points, and libatx's (include/atx.h, ATX_VERSION 420), are fixed, tested sets.
 * The libraries share no symbol and no state; this header includes atx.h for the status codes, atx_dtype and atx_layout, which mean
 * here what they mean there.
 *
 * Conventions (atx.h states them in full; they hold unchanged)
 *  - Plain C types only.  Every pointer named in a signature is a DEVICE pointer (HBM): NO pointer here is a host pointer.  The caller
 *    owns every buffer; the library keeps no state besides a thread-local error string.  A buffer of ZERO elements may be NULL.
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls enqueue work and return without synchronising.
 *  - Return value: ATX_OK (0) or a negative ATX_E* code; atx_pltz_last_error() gives the message for the calling thread.
 *  - Every entry point is re-entrant.
 */
#ifndef ATX_PLTZ_H
#define ATX_PLTZ_H

#include <stddef.h>
#include <stdint.h>

#include "atx.h"

/* Built with -fvisibility=hidden and a version script made from this header: the ATX_PLTZ_API declarations below are the library's
 * ONLY dynamic symbols (tests/test_host_api.py checks `nm -D --defined-only` against this header). */
#if defined(_WIN32)
#define ATX_PLTZ_API
#else
#define ATX_PLTZ_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define ATX_PLTZ_VERSION 420 /* goes with ATX_VERSION */

#define ATX_PLTZ_MAX_LEVELS 256 /* rows of t and of q that one call takes (ATX_HEIGHTS_MAX_LEVELS); more is ATX_ENOTIMPL */

/* ATX_PLTZ_VERSION of the library that was loaded. */
ATX_PLTZ_API int atx_pltz_version(void);

/* The message of the last failed call of the calling thread ("" if none); valid until that thread's next failing call. */
ATX_PLTZ_API const char* atx_pltz_last_error(void);

/*
 * Temperature and geopotential on pressure levels, and mean sea level pressure.  For one grid point: the surface pressure sp (Pa), the
 * surface geopotential zs (m^2/s^2), the half-level coefficients A[0..H-1], B[0..H-1] (H = n_half) and the n = n_lev rows t[0..n-1] (K),
 * q[0..n-1] (kg/kg), top first.  The rows are the LOWEST n model levels: row k is the 0-based model level j = first + k with
 * first = H - 1 - n, the rule of atx_heights_interpolate.  A target P is a pressure in Pa.  All arithmetic is in float64 for both
 * storage widths, one IEEE operation at a time, without contraction, with IEEE divisions and the library's own logarithm and
 * exponential (<= 1 ulp each); every parenthesis below is one operation, sums and products without one go from left to right; the
 * result is rounded once at the store.  Constants: g = 9.80665, Rd = 287.0597, Rv = 461.5250, gamma = 0.0065 K/m,
 * kappa = (gamma * Rd) / g.
 *     p_half(j) = A[j] + B[j] * sp;   p[k] = (p_half(first + k) + p_half(first + k + 1)) / 2.0;   p_g = p_half(H - 1)   (the ground)
 *     c[k]: the hydrostatic geopotential of full level k, exactly c[k] of atx_heights.h with z0 = zs:
 *         S = 0.0;  for k = n - 1 down to 0, j = first + k:
 *             p_up = p_half(j);  p_dn = p_half(j + 1);  r = Rd * (1.0 - q[k]) + Rv * q[k]
 *             j == 0:  alpha = 0.6931471805599453;  no delta
 *             j  > 0:  delta = log(p_dn / p_up);   alpha = 1.0 - p_up / (p_dn - p_up) * delta
 *             c[k] = zs + (S + (alpha * r) * t[k]);      j > 0:  S = S + (delta * r) * t[k]
 *     L = n - 1;   coord(p) = p (ATX_PLTZ_LINEAR)  or  log(p) (ATX_PLTZ_LOG)
 * Per point, with no library function involved:
 *     hgt = zs / g
 *     T*  = t[L] + (kappa * t[L]) * (p_g / p[L] - 1.0)
 *     T0  = T* + gamma * hgt
 *     aZ = kappa, Tz = T*                                                            (what z and msl extrapolate with)
 *     T* <= 290.5 and T0 > 290.5:   aZ = (Rd * (290.5 - T*)) / zs
 *     T*  > 290.5 and T0 > 290.5:   aZ = 0.0,  Tz = 0.5 * (290.5 + T*)
 *     then, in every case,  Tz < 255.0:   Tz = 0.5 * (255.0 + Tz)
 * Per target P, with i = #{k : p[k] <= P}, counted over the WHOLE column, the first rule that applies:
 *  1. sp != sp or zs != zs        every output of the point is NaN, msl included
 *  2. i == 0                      (above the top full level)  t = z = NaN
 *  3. 0 < i < n                   a = i - 1, b = i;  w = (coord(P) - coord(p[a])) / (coord(p[b]) - coord(p[a]))
 *                                 y = x[a] + w * (x[b] - x[a])          for x = t and for x = c
 *  4. i == n and P <= p_g         (the lowest half layer)  w = (coord(P) - coord(p[L])) / (coord(p_g) - coord(p[L]))
 *                                 y = x[L] + w * (x_s - x[L]),   x_s = T* for t,  x_s = zs for z
 *  5. i == n and P > p_g          (under the ground)  l = log(P / p_g)
 *        temperature:   hgt < 2000.0:    y = kappa * l
 *                       otherwise        Tplat = T0 < 298.0 ? T0 : 298.0
 *                                        hgt > 2500.0:  T0' = Tplat
 *                                        else           T0' = 0.002 * ((2500.0 - hgt) * T0 + (hgt - 2000.0) * Tplat)
 *                                        T0' < T*:  y = 0.0;   else  y = ((Rd * (T0' - T*)) / zs) * l
 *                       y2 = y * y;  y3 = y2 * y;   t = T* * (((1.0 + y) + y2 / 2.0) + y3 / 6.0)
 *        geopotential:  y = aZ * l;   z = zs - ((Rd * Tz) * l) * ((1.0 + y / 2.0) + (y * y) / 6.0)
 *     (i == n with neither P <= p_g nor P > p_g — a NaN p_g from the table — is NaN.)
 *  6. msl, once per point:        |zs| < 0.001:  msl = p_g
 *                                 otherwise  h = zs / (Rd * Tz);  x = (aZ * zs) / (Rd * Tz)
 *                                            msl = p_g * exp(h * ((1.0 - x / 2.0) + (x * x) / 3.0))
 * So: every branch is decided on values that involve no library function — a restatement in another IEEE arithmetic that keeps this
 * order takes the same branch for every input; in the linear coordinate the interior t has no library function in it at all and is
 * what atx_levels_interpolate gives, bit for bit; a target exactly on a full level has w == 0 and returns x[a]; under the ground with
 * hgt > 2500 and T0' < T* the temperature is T* exactly; a NaN in t or q at level k makes c NaN at k and above and reaches t only
 * through its bracket; a NaN t[L] makes T*, and with it msl and everything under the ground, NaN.  Which NaN is written is
 * unspecified.  This is the ECMWF post-processing scheme as Trenberth, Berry and Buja (1993, NCAR/TN-396) write it, restated here;
 * parity with IFS / MARS is unpinned.
 *
 *   t, q      n_lev rows each;  t_pitch, q_pitch per stack
 *   out       2 * n_tgt rows, or 2 * n_tgt + 1 with msl != 0: row i is t at targets[i], row n_tgt + i is z at targets[i], row 2 * n_tgt
 *             is msl
 *   All three stacks hold n_pts points in ONE dtype and ONE layout; pitches in elements: between points (ATX_COLUMNS: >= the stack's
 *   rows) or between rows (ATX_FIELDS: >= n_pts).
 *   sp, zs    [n_pts] each, the stacks' type
 *   A, B      float64 [n_half];  targets  float64 [n_tgt], Pa: any order, duplicates allowed, the output is in the given order
 * Both layouts and every load route give the same bits.  ATX_COLUMNS: a workgroup stages the t and q columns of a run of consecutive
 * points in LDS (16-byte vectors where base, pitch and the column's last vector allow, decided per stack; reads may cover the pitch
 * padding inside that vector, nothing beyond), computes the terms with one lane per (point, level), sums per point over LDS, computes
 * the per-point quantities and msl with one lane per point, both outputs of a target with one lane per (point, target), and writes a
 * point's rows as one run.  ATX_FIELDS: one lane per point.  The padding of out is not written; t, q, sp and zs are not modified.
 *
 * Validation comes before anything touches HIP.  ATX_EINVAL: an unknown dtype, layout or coordinate, msl other than 0 / 1; n_pts < 0,
 * n_lev < 1, n_tgt < 0, n_half < 2, n_lev > n_half - 1; a NULL pointer for a buffer that is not empty; out's extent overlapping t's, q's,
 * sp's or zs'.  ATX_ESHAPE: a pitch too small for the shape.  ATX_ENOTIMPL: n_lev > ATX_PLTZ_MAX_LEVELS, n_pts beyond int32, n_half or
 * 2 * n_tgt + 1 beyond 65535, or (ATX_COLUMNS) one point's columns and outputs beyond the LDS of a workgroup — never a silently wrong
 * result.  No points, or no targets and no msl: ATX_OK, nothing is launched; no targets with msl: the launch writes msl.
 */
typedef enum { ATX_PLTZ_LINEAR = 0, ATX_PLTZ_LOG = 1 } atx_pltz_coordinate;
ATX_PLTZ_API int atx_pltz_interpolate(const void* t, const void* q, const void* sp, const void* zs, void* out, const double* A,
                                      const double* B, const double* targets, int64_t n_pts, int64_t n_lev, int64_t n_tgt,
                                      int64_t n_half, int64_t t_pitch, int64_t q_pitch, int64_t out_pitch, int dtype, int layout,
                                      int coordinate, int msl, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* ATX_PLTZ_H */
