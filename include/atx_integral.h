/*
 * atx_integral.h — C ABI of libatx_integral, the vertical REDUCTION that goes with libatx (MI355X, gfx950): pressure-weighted column
 * integrals and layer means of the variables of a stack of levels — total column water vapour 1/g ∫ q dp, the integrated vapour
 * transport 1/g ∫ q u dp and 1/g ∫ q v dp, the mass-weighted mean of r between 850 and 500 hPa — on hybrid model levels or on pressure
 * levels.  libatx_levels, libatx_geopotential, libatx_heights, libatx_pltz and libatx_coord move values from one level to another;
 * this library reduces a column to one value per (term, bound).
 *
 * A companion library with its own header, as libatx_text, libatx_plan, libatx_mesh, libatx_missing, libatx_stat, libatx_levels,
 * libatx_geopotential, libatx_heights, libatx_pltz and libatx_coord are: libatx's entry points are a fixed, tested set (include/atx.h,
 * ATX_VERSION 420).  The libraries share no symbol and no state; this header includes atx.h for the status codes, atx_dtype and
 * atx_layout, which mean here what they mean there.
 *
 * Conventions (atx.h states them in full; they hold unchanged)
 *  - Plain C types only.  Every pointer named in a signature is a DEVICE pointer (HBM) — except `terms` and `bounds`, which are HOST
 *    arrays: they are validated before anything is launched and travel with the launch.  The caller owns every buffer; the library
 *    keeps no state besides a thread-local error string.  A buffer of ZERO elements may be NULL.
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls enqueue work and return without synchronising.
 *  - Return value: ATX_OK (0) or a negative ATX_E* code; atx_integral_last_error() gives the message for the calling thread.
 *  - Every entry point is re-entrant.
 */
#ifndef ATX_INTEGRAL_H
#define ATX_INTEGRAL_H

#include <stddef.h>
#include <stdint.h>

#include "atx.h"

/* Built with -fvisibility=hidden and a version script made from this header: the ATX_INTEGRAL_API declarations below are the
 * library's ONLY dynamic symbols (tests/test_host_api.py checks `nm -D --defined-only` against this header). */
#if defined(_WIN32)
#define ATX_INTEGRAL_API
#else
#define ATX_INTEGRAL_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define ATX_INTEGRAL_VERSION 420 /* goes with ATX_VERSION */

#define ATX_INTEGRAL_MAX_LEVELS 256 /* rows per variable that one call takes; more is ATX_ENOTIMPL */
#define ATX_INTEGRAL_MAX_TERMS 64   /* terms of one call; more is ATX_ENOTIMPL */
#define ATX_INTEGRAL_MAX_BOUNDS 32  /* bounds of one call; more is ATX_ENOTIMPL */

/* The block length of the sum.  It is part of the statement: it fixes the order of the additions and with it the bits. */
#define ATX_INTEGRAL_BLOCK 8

/* The gravitational acceleration the integral is divided by (m / s^2). */
#define ATX_INTEGRAL_G 9.80665

/* How far a result can lie from the statement in exact arithmetic on the same inputs, in float64 ulps of S = sum |w_k f_k| / divisor
 * (the derivation is below): n_lev levels, K = max P / min dP.  A float32 stack adds its one rounding at the store:
 * 0.5 + ATX_INTEGRAL_ULPS_F64(...) * 2^-29 float32 ulps.  A mean divides two such sums: twice the bound. */
#define ATX_INTEGRAL_ULPS_F64(n_lev, K) \
    (16.0 * (K) + ATX_INTEGRAL_BLOCK + ((n_lev) + ATX_INTEGRAL_BLOCK - 1) / ATX_INTEGRAL_BLOCK + 2)

/* ATX_INTEGRAL_VERSION of the library that was loaded. */
ATX_INTEGRAL_API int atx_integral_version(void);

/* The message of the last failed call of the calling thread ("" if none); valid until that thread's next failing call. */
ATX_INTEGRAL_API const char* atx_integral_last_error(void);

/*
 * Column integrals and layer means.  For one grid point p: n_var variable columns x[v][0..n-1] of n = n_lev levels, top level first,
 * in the storage type T (float32 or float64), and the surface pressure sp[p] in T.  bounds[b] = (top, bottom) in Pa, float64,
 * 0 <= top < bottom, bottom may be +inf.  terms[t] = (v1, v2): the integrand at level k is f_k = (double)x[v1][k], or, where v2 >= 0,
 * the float64 product (double)x[v1][k] * (double)x[v2][k], rounded once.  Everything below is float64, one IEEE operation at a time,
 * without contraction; every max and min is a comparison and a select, so no NaN depends on a library's fmax.
 *
 *   Weights.  For every (point, bound) a weight w_k per level, shared by all terms.
 *     ATX_INTEGRAL_HYBRID   model levels; A, B: the n + 1 half levels of the rows (a run of the model's table, which need not reach
 *                           the ground).  lo = A[k] + B[k] * sp, hi = A[k+1] + B[k+1] * sp;  a = lo > top ? lo : top;
 *                           c = hi < bottom ? hi : bottom;  w_k = c > a ? c - a : 0.  The value is constant in its layer: the
 *                           finite-volume sum of IFS.
 *     ATX_INTEGRAL_PRESSURE pressure levels P[0] < ... < P[n-1] (Pa).  m = #{k : P[k] <= sp} levels are above the ground; the column
 *                           lives on [P[0], sp].  Between two levels above the ground the value is linear in p: segment j
 *                           (j + 1 < m), clipped to a = P[j] > top ? P[j] : top, c = P[j+1] < bottom ? P[j+1] : bottom, gives, where
 *                           c > a:  len = c - a;  mid = (a + c) / 2;  r = (mid - P[j]) / (P[j+1] - P[j]);  len * (1 - r) to w_j and
 *                           len * r to w_{j+1} — the trapezoid of the clipped segment.  The lowest level above the ground holds its
 *                           value down to the ground: the segment [P[m-1], sp], clipped the same way, gives c - a to w_{m-1} where
 *                           c > a.  w_k = (share of the segment above, k - 1) + (share of the segment below, k), in that order, an
 *                           absent share being +0.0.  Levels under the ground (k >= m) have w_k = 0 exactly and are never read as
 *                           values: archives hold NaN or extrapolated numbers there.
 *   Sum.      A level with w_k == 0 is skipped, whatever its value (NaN included).  The others contribute fl(w_k * f_k).
 *             ATX_INTEGRAL_BLOCK consecutive levels (the last block may be short) are added in ascending order into a block sum that
 *             starts at +0.0; the block sums are added in ascending order into acc, which starts at +0.0.  wsum is formed the same way
 *             from the weights themselves.
 *   Result.   ATX_INTEGRAL_SUM: acc / 9.80665.  ATX_INTEGRAL_MEAN: acc / wsum — an empty layer is 0 / 0 = NaN, an empty SUM is 0.
 *             A NaN sp makes every result of the point NaN.  The result is rounded once to T.  Which NaN is written is unspecified.
 *   Parity.   The hybrid sum is IFS' own finite-volume column integral and earthkit-meteo's; parity is unpinned.
 *
 * Accuracy (ATX_INTEGRAL_ULPS_F64).  u = 2^-53, every operation rounded once, no overflow and no subnormal.  "max P": the largest
 * finite pressure that enters a weight (a half level, a level, sp, a finite bound); "min dP": the smallest non-zero weight of the
 * (point, bound), in either arithmetic; K = max P / min dP.
 *   Weights, HYBRID.   lo and hi carry two roundings each: |d lo|, |d hi| <= 2 u max P.  Clipping (a select of two values) is
 *     1-Lipschitz, so a and c move by no more, whichever side the selects fall on in either arithmetic, and the subtraction adds one
 *     rounding: |w_k - w*_k| <= 4 u max P + u w_k <= (4 K + 1) u w_k.
 *   Weights, PRESSURE.  a and c are inputs: exact, and so is m.  len has one rounding.  mid has one (the halving is exact):
 *     |d mid| <= u max P.  mid - P[j] adds one, the span P[j+1] - P[j] has one, the division one: with 0 <= r <= 1 and span >= len,
 *     |d r| <= u max P / span + 3 u.  1 - r adds one rounding, each product one: |d share| <= len (u max P / span + 6 u)
 *     <= u max P + 6 u len, two shares and their sum: |w_k - w*_k| <= 2 u max P + 12 u max P + u w_k <= (14 K + 1) u w_k.
 *   Both are within (16 K + 1) u w_k.  f_k has at most one rounding and the product w_k f_k one:
 *     fl(w_k f_k) = w*_k f*_k (1 + t), |t| <= (16 K + 3) u.
 *   Sum.  A term passes at most BLOCK - 1 additions inside its block (the first is to +0.0: exact) and at most
 *     ceil(n / BLOCK) - 1 additions of block sums; the division adds one rounding:
 *     |y - y*| <= (16 K + 3 + BLOCK - 1 + ceil(n / BLOCK) - 1 + 1) u S = (16 K + BLOCK + ceil(n / BLOCK) + 2) u S,
 *     and u S is less than one ulp of S.  With the block length 8 and 137 levels the sum contributes 26 of these ulps, where one
 *     running sum would contribute 137.
 *   Mean.  wsum is such a sum of positive terms, so relative to itself; the quotient of the two carries both errors: at most
 *     twice the bound, in ulps of sum |w_k f_k| / wsum.
 *
 *   src       n_var variables x n_lev rows each, variables adjacent (rows v * n_lev .. v * n_lev + n_lev - 1 are variable v), n_pts points
 *   sp        [n_pts] in the stack's type
 *   out       n_term x n_bnd rows (row t * n_bnd + b is term t over bounds[b]), n_pts points, the layout and type of src
 *   terms     HOST int32 [n_term][2]: (v1, v2), 0 <= v1 < n_var, v2 < n_var, v2 < 0: no second factor
 *   bounds    HOST float64 [n_bnd][2]: (top, bottom) in Pa
 *   A, B      float64 [n_lev + 1] (ATX_INTEGRAL_HYBRID; levels_pa is ignored)
 *   levels_pa float64 [n_lev], strictly increasing (ATX_INTEGRAL_PRESSURE; A and B are ignored).  It is device memory: its order is the
 *             caller's to keep
 *   src_pitch, out_pitch   in elements: between points (ATX_COLUMNS: >= n_var * n_lev, >= n_term * n_bnd) or between rows
 *             (ATX_FIELDS: >= n_pts)
 * Both layouts give the same bits.  ATX_COLUMNS: a 256-lane workgroup per tile of consecutive points stages their columns in LDS with
 * loads that cover the run contiguously — 16-byte vectors where the base is 16-byte aligned, the pitch a multiple of 16 bytes and the
 * last vector of a column inside the pitch (reads may cover the pitch padding inside that vector, nothing beyond), single elements
 * otherwise — forms the weights once per (point, bound, level), the block sums with one lane per (point, bound, term, block), and
 * writes each point's outputs as one contiguous run.  ATX_FIELDS: one lane per (point, bound), the rows read coalesced.
 *
 * Validation comes before anything touches HIP.  ATX_EINVAL: an unknown dtype, layout, mode or kind; n_pts < 0, n_var < 1, n_lev < 1,
 * n_term < 0, n_bnd < 0; a term index outside the variables; a bound that is not 0 <= top < bottom; a NULL pointer for a buffer that
 * is not empty; an out that overlaps src or sp.  ATX_ESHAPE: a pitch too small for the shape.  ATX_ENOTIMPL: n_lev, n_term or n_bnd
 * beyond the caps above, sizes beyond int32, or (ATX_COLUMNS) one point's rows, weights and block sums beyond the LDS of a workgroup —
 * never a silently wrong result.  No points, no terms or no bounds: ATX_OK, nothing is launched.
 */
typedef enum { ATX_INTEGRAL_HYBRID = 0, ATX_INTEGRAL_PRESSURE = 1 } atx_integral_mode;
typedef enum { ATX_INTEGRAL_SUM = 0, ATX_INTEGRAL_MEAN = 1 } atx_integral_kind;
ATX_INTEGRAL_API int atx_integral_columns(const void* src, const void* sp, void* out, const int32_t* terms, const double* bounds, const double* A,
                                          const double* B, const double* levels_pa, int64_t n_pts, int64_t n_var, int64_t n_lev, int64_t n_term,
                                          int64_t n_bnd, int64_t src_pitch, int64_t out_pitch, int dtype, int layout, int mode, int kind, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* ATX_INTEGRAL_H */
