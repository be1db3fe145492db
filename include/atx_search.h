/*
 * atx_search.h — C ABI of libatx_search, the column SEARCH that goes with libatx (MI355X, gfx950): the first step of a column, read from
 * the ground or from the top, at which a search variable crosses a value — the freezing level where the column has inversions, the
 * dynamic tropopause, cloud base and cloud top — or the level of its maximum or minimum — the jet level, the warmest level of an
 * inversion — and the variables of a stack there.  libatx_coord interpolates on a coordinate column that is strictly MONOTONE and refuses
 * every other; here a column is whatever it is: nothing is checked, nothing is bisected, the answer is the first step in scan order that
 * satisfies a predicate, or the first arg-extremum.
 *
 * A companion library with its own header, as libatx_text, libatx_plan, libatx_mesh, libatx_missing, libatx_stat, libatx_levels,
 * libatx_geopotential, libatx_heights, libatx_pltz, libatx_coord and libatx_integral are: libatx's entry points are a fixed, tested set
 * (include/atx.h, ATX_VERSION 420).  The libraries share no symbol and no state; this header includes atx.h for the status codes,
 * atx_dtype and atx_layout, which mean here what they mean there.
 *
 * Conventions (atx.h states them in full; they hold unchanged)
 *  - Plain C types only.  Every pointer named in a signature is a DEVICE pointer (HBM).  The caller owns every buffer; the library
 *    keeps no state besides a thread-local error string.  A buffer of ZERO elements may be NULL.
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls enqueue work and return without synchronising.
 *  - Return value: ATX_OK (0) or a negative ATX_E* code; atx_search_last_error() gives the message for the calling thread.
 *  - Every entry point is re-entrant.
 */
#ifndef ATX_SEARCH_H
#define ATX_SEARCH_H

#include <stddef.h>
#include <stdint.h>

#include "atx.h"

/* Built with -fvisibility=hidden and a version script made from this header: the ATX_SEARCH_API declarations below are the
 * library's ONLY dynamic symbols (tests/test_host_api.py checks `nm -D --defined-only` against this header). */
#if defined(_WIN32)
#define ATX_SEARCH_API
#else
#define ATX_SEARCH_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define ATX_SEARCH_VERSION 420 /* goes with ATX_VERSION */

#define ATX_SEARCH_MAX_LEVELS 256 /* rows per variable that one call takes; more is ATX_ENOTIMPL */

/* The accuracy of a crossing's result against the statement in exact arithmetic on the same inputs, in float64 ulps of
 * max(|x[a]|, |x[b]|) (the derivation is below).  A float32 stack adds its one rounding at the store: 0.5 + 11 * 2^-29 float32 ulps. */
#define ATX_SEARCH_ULPS_F64 11

/* ATX_SEARCH_VERSION of the library that was loaded. */
ATX_SEARCH_API int atx_search_version(void);

/* The message of the last failed call of the calling thread ("" if none); valid until that thread's next failing call. */
ATX_SEARCH_API const char* atx_search_last_error(void);

/*
 * The search of a column.  For one grid point p: the n = n_lev rows s[0..n-1] of the search column, the rows x_v[0..n-1] of n_var >= 0
 * variables on the same rows, and level_values[0..n-1], an optional float64 array that is the same for every point: where it is given
 * it is one more variable, the LAST ("at which pressure / level"), interpolated in float64 as the others are.  e, x: the columns read
 * in SCAN order — ATX_SEARCH_FORWARD reads row 0 first (e[k] = s[k]), ATX_SEARCH_BACKWARD reads row n - 1 first (e[k] = s[n - 1 - k]).
 * All arithmetic is in float64 for both storage widths, one operation at a time, without contraction, with IEEE divisions; the result
 * is rounded once at the store.  No mode checks that a column is monotone and none reports a bad point.
 *
 *   Crossing modes, for the targets T = targets[t].  Step k (0 <= k < n - 1) is
 *               an UP crossing     where  e[k] <= T && T <  e[k+1]
 *               a DOWN crossing    where  e[k] >= T && T >  e[k+1]
 *             ATX_SEARCH_UP asks for the first kind, ATX_SEARCH_DOWN for the second, ATX_SEARCH_ANY for either ("rising" and "falling"
 *             are read ALONG THE SCAN).  The answer is the FIRST such k in scan order:
 *               a = k, b = k + 1;  w = (T - e[a]) / (e[b] - e[a]);  y_v = x_v[a] + w * (x_v[b] - x_v[a])
 *             One compare of every crossing is strict, so the denominator is never zero and w is in [0, 1).  A target exactly on level
 *             a has w == 0 and returns x[a] + 0 * (x[b] - x[a]): that level's bits for every finite bracket (+0.0 for -0.0).
 *               no step crosses and e[n-1] == T   y_v = x_v[n-1] (of the scan: the last row read), that row's bits
 *               otherwise                         every output of the (point, target) pair is NaN
 *             A NaN in e makes both steps that touch it non-crossings — every compare with it is false — so a run of NaN under the
 *             ground on pressure levels is skipped, not fatal.  A NaN target crosses nothing and equals nothing.  An infinity in e is
 *             an ordinary value of the compares, and the result is the plain result of the formula: a bracket from -inf or to +inf
 *             crossed UP (from +inf or to -inf crossed DOWN) has an infinite denominator, so w is NaN where the numerator is infinite
 *             too (e[a] infinite) and 0 where only e[b] is — then y_v = x_v[a] + 0 * (x_v[b] - x_v[a]).  A NaN in x reaches only the
 *             targets whose bracket holds it.  Which NaN is written is unspecified.
 *             count[p * n_tgt + t] (ATX_COLUMNS; [t * n_pts + p] in ATX_FIELDS): the number of steps of the asked kind in the WHOLE
 *             column, saturating at 255.  0: no crossing (the e[n-1] == T row is not one);  above 1: the first is not the only one.
 *   Extremum modes (ATX_SEARCH_MAX, ATX_SEARCH_MIN;  n_tgt must be 1 and `targets` is ignored).
 *               a = the first k in scan order with e[k] equal to the maximum (minimum) over the entries of e that are not NaN
 *               y_v = x_v[a], that row's bits: no interpolation (level_values[a] is rounded to the stack's type)
 *               every e[k] NaN: y_v = NaN
 *             -0.0 and +0.0 are equal.  count[p]: the number of rows equal to the extremum, saturating at 255 (0: all NaN).
 *   The step and w of a (point, target) pair are computed once and applied to all variables.
 *   Parity.   The statement is in-tree and UNPINNED against earthkit-meteo and IFS; IFS's own freezing level (deg0l) has further rules
 *             for a second warm layer which are not applied here.
 *
 * Accuracy of a crossing (ATX_SEARCH_ULPS_F64).  The derivation of atx_coord.h holds with N = T - e[a] and D = e[b] - e[a] of either
 * common sign (UP: 0 <= N < D;  DOWN: D < N <= 0).  With u = 2^-53 and every operation rounded once: fl(N) = N (1 + e1),
 * fl(D) = D (1 + e2), w = fl(N) / fl(D) (1 + e3), fl(x[b] - x[a]) = (x[b] - x[a]) (1 + e4), s = w fl(x[b] - x[a]) (1 + e5) =
 * (N / D) (x[b] - x[a]) (1 + theta) with |theta| <= 5 u + O(u^2), and y = (x[a] + s) (1 + e6): six roundings.  The exact
 * y* = x[a] + (N / D) (x[b] - x[a]) lies between x[a] and x[b], so with M = max(|x[a]|, |x[b]|): |y*| <= M and
 * |(N / D) (x[b] - x[a])| <= 2 M, hence |y - y*| <= 5 u 2 M + u M + O(u^2) = 11 u M, and u M is less than one ulp of M.  The bound
 * supposes that no intermediate overflows or is subnormal.  An extremum copies bits.
 *
 *   src           n_var variables x n_lev rows each, variables adjacent (rows v * n_lev .. v * n_lev + n_lev - 1 are variable v), n_pts
 *                 points; NULL where n_var == 0
 *   search        n_lev rows: the search variable of every row at every point, in the layout and type of src
 *   out           (n_var + has_level_values) x n_tgt rows (row v * n_tgt + t is variable v at targets[t]), n_pts points, the layout
 *                 and type of src; NULL where there is no such row
 *   count         uint8 [n_pts x n_tgt] as stated above, or NULL; written for every (point, target) with plain vector stores, no atomics
 *   targets       float64 [n_tgt]: any order, duplicates allowed, the output is in the given order (extremum modes: ignored, may be NULL)
 *   level_values  float64 [n_lev] or NULL
 *   src_pitch, search_pitch, out_pitch   in elements: between points (ATX_COLUMNS: >= n_var * n_lev, >= n_lev, >= the rows of out) or
 *                 between rows (ATX_FIELDS: >= n_pts)
 * Both layouts give the same bits.  ATX_COLUMNS: a workgroup stages the search columns and the variable columns of a run of consecutive
 * points in LDS with loads that cover the run contiguously — each of the two stacks on its own route: 16-byte vectors where its base is
 * 16-byte aligned, its pitch a multiple of 16 bytes and the last vector of a column inside the pitch (reads may cover the pitch padding
 * inside that vector, nothing beyond), single elements otherwise; both routes give the same bits.  The search is wave-cooperative: the
 * lanes of a wave are the STEPS of a column, a ballot gives their predicates as a mask, its first or last bit is the answer; columns of
 * 32 levels or fewer share a wave.  Each point's outputs are written as one contiguous run.  ATX_FIELDS: one lane per (point, target),
 * the rows read strided in scan order.
 *
 * Validation comes before anything touches HIP.  ATX_EINVAL: an unknown dtype, layout, direction or mode; n_pts < 0, n_var < 0,
 * n_lev < 1, n_tgt < 0; an extremum mode with n_tgt > 1; n_var == 0 without level_values and without count (nothing would be written);
 * a NULL pointer for a buffer that is not empty; an out or a count that overlaps an input, or each other.  ATX_ESHAPE: a pitch too
 * small for the shape.  ATX_ENOTIMPL: n_lev > ATX_SEARCH_MAX_LEVELS, sizes beyond int32, or (ATX_COLUMNS) one point's columns and
 * outputs beyond the LDS of a workgroup — never a silently wrong result.  No points or no targets: ATX_OK, nothing is launched.
 */
typedef enum { ATX_SEARCH_FORWARD = 0, ATX_SEARCH_BACKWARD = 1 } atx_search_direction;
typedef enum { ATX_SEARCH_UP = 0, ATX_SEARCH_DOWN = 1, ATX_SEARCH_ANY = 2, ATX_SEARCH_MAX = 3, ATX_SEARCH_MIN = 4 } atx_search_mode;
ATX_SEARCH_API int atx_search_columns(const void* src, const void* search, void* out, uint8_t* count, const double* targets,
                                      const double* level_values, int64_t n_pts, int64_t n_var, int64_t n_lev, int64_t n_tgt, int64_t src_pitch,
                                      int64_t search_pitch, int64_t out_pitch, int dtype, int layout, int direction, int mode, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* ATX_SEARCH_H */
