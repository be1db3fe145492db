/*
 * atx_parcel.h — C ABI of libatx_parcel, the parcel ascent that goes with libatx (MI355X, gfx950): CAPE, CIN and the lifting
 * condensation level of every column of a stack of temperature and specific humidity, on hybrid model levels or on pressure levels.
 * The other vertical libraries move values between levels (libatx_levels, libatx_geopotential, libatx_heights, libatx_pltz,
 * libatx_coord), sum a column (libatx_integral) or search it (libatx_search); this one follows an air parcel through it.
 *
 * A companion library with its own header, as the thirteen others are: libatx's entry points are a fixed, tested set (include/atx.h,
 * ATX_VERSION 420).  The libraries share no symbol and no state; this header includes atx.h for the status codes, atx_dtype and
 * atx_layout, which mean here what they mean there.
 *
 * Conventions (atx.h states them in full; they hold unchanged)
 *  - Plain C types only.  Every pointer named in a signature is a DEVICE pointer (HBM).  The caller owns every buffer; the library
 *    keeps no state besides a thread-local error string.  A buffer of ZERO elements may be NULL.
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls enqueue work and return without synchronising.
 *  - Return value: ATX_OK (0) or a negative ATX_E* code; atx_parcel_last_error() gives the message for the calling thread.
 *  - Every entry point is re-entrant.
 */
#ifndef ATX_PARCEL_H
#define ATX_PARCEL_H

#include <stddef.h>
#include <stdint.h>

#include "atx.h"

/* Built with -fvisibility=hidden and a version script made from this header: the ATX_PARCEL_API declarations below are the
 * library's ONLY dynamic symbols (tests/test_host_api.py checks `nm -D --defined-only` against this header). */
#if defined(_WIN32)
#define ATX_PARCEL_API
#else
#define ATX_PARCEL_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define ATX_PARCEL_VERSION 420 /* goes with ATX_VERSION */

#define ATX_PARCEL_MAX_LEVELS 256 /* levels that one call takes; more is ATX_ENOTIMPL */
#define ATX_PARCEL_OUTPUTS 5      /* rows of `out`: cape, cin, plcl, tlcl, pstart, in this order */

/* The block length of the two sums.  It is part of the statement: it fixes the order of the additions and with it the bits. */
#define ATX_PARCEL_BLOCK 8

/* The Newton steps of the moist adiabat.  The count is FIXED and part of the statement: the smallest count after which one more
 * step moves T by less than one float64 ulp.  The sweep that gave it (tools/parcel_newton_sweep.py), on the CPU, in 80-bit extended arithmetic so that the step
 * and not its rounding is measured: starts at p_s = 1080, 1000, 850, 700, 500 and 300 hPa, T_s = 230 .. 320 K every 0.5 K,
 * relative humidity 1, 0.999, 0.9, 0.5, 0.1, 1e-3 and 1e-6, 400 levels from p_s to 50 hPa in equal steps of ln p, every level above
 * the LCL solved from the dry-adiabat value: step 10 still moves T by an ulp or more at 1835 of 2.4 million levels (all of them
 * of the starts at 500 and 300 hPa), step 11 at none; 9 steps suffice for every start at 700 hPa or nearer the ground, and 94 % of
 * the levels need 7 or fewer.  The cap of a step (below) was met 117 751 times in these 24 million steps. */
#define ATX_PARCEL_NEWTON_STEPS 10

/* ATX_PARCEL_VERSION of the library that was loaded. */
ATX_PARCEL_API int atx_parcel_version(void);

/* The message of the last failed call of the calling thread ("" if none); valid until that thread's next failing call. */
ATX_PARCEL_API const char* atx_parcel_last_error(void);

/*
 * The ascent of one parcel per column.  For one grid point: the columns t[k] (K) and q[k] (kg / kg) of n = n_lev levels, top level
 * first, in the storage type T (float32 or float64), and the surface pressure sp in T.  Everything below is float64, one IEEE
 * operation at a time, without contraction, in the order the parentheses give; every max and min is a comparison and a select; log
 * and exp are the natural ones.  Each result is rounded once to T.  Which NaN is written is unspecified.
 *
 *   Constants.  Rd = 287.0597, Rv = 461.5250 (atx_geopotential.h), eps = Rd / Rv, kappa = 2 / 7, L5 = 11.512925464970229 (ln 10^5).
 *     es(T) = 611.21 exp((17.502 (T - 273.16)) / (T - 32.19)): the saturation pressure over water of the humidity operators of libatx.
 *   Levels.   ATX_PARCEL_HYBRID: A, B are the n + 1 half levels of the rows, p_k = ((A[k] + B[k] sp) + (A[k+1] + B[k+1] sp)) / 2.
 *     ATX_PARCEL_PRESSURE: p_k = levels_pa[k], strictly increasing.  Level k takes part where p_k >= p_top and, on pressure levels,
 *     p_k <= sp: the levels under the ground are never used as values — archives hold NaN or extrapolated numbers there — and
 *     nothing of them shows.  kt is the first, kb the last level that takes part (p_k increases with k: on hybrid levels that is the
 *     caller's table to keep).  A NaN sp, no level that takes part, or a NaN in t or q at one of the levels kt .. kb: every output of
 *     the point is NaN.  q outside [0, 1) or t <= 0 there: unspecified.
 *   Parcel of level k.  r = q / (1 - q);  e = (p r) / (eps + r);  lnT = log(T);
 *     T_L = 2840 / ((3.5 lnT - log(e / 100)) - 4.805) + 55                                                  (Bolton 1980, eq. 21)
 *     ln theta_e = H(lnT, T_L, r, ln p) = (lnT + (0.2854 (1 - 0.28 r)) (L5 - ln p)) + ((3.376 / T_L - 0.00254) (1000 r)) (1 + 0.81 r)
 *                                                                            (eq. 43, its logarithm: theta_e itself is never formed)
 *   Start level s.  ATX_PARCEL_LOWEST: s = kb.  ATX_PARCEL_MOST_UNSTABLE: among the levels kt .. kb with p_k >= p_kb - depth the
 *     one of the largest ln theta_e; among equals the nearest to the ground.  pstart = p_s, tlcl = T_L of s,
 *     plcl = p_L = p_s exp(3.5 log(T_L / T_s)).
 *   Parcel temperature at a level k, kt <= k < s.  The dry adiabat Td = T_s exp(kappa log(p_k / p_s)).  Where p_k >= p_L the parcel is
 *     (Td, r_s).  Elsewhere it is saturated, (T, r(T)), T the root of H(log T, T, r(T), ln p_k) = ln theta_e of s with
 *     es = es(T), pe = p_k - es, r(T) = (eps es) / pe, found by ATX_PARCEL_NEWTON_STEPS Newton steps from Td:
 *       F = H(log T, T, r, ln p_k) - ln theta_e;   d = T - 32.19;   dr = (r (p_k / pe)) (4217.45694 / (d d));   w = (1000 r)(1 + 0.81 r)
 *       F' = ((1 / T - (0.079912 dr)(L5 - ln p_k)) - (3.376 / (T T)) w) + ((3.376 / T - 0.00254)(1000 dr))(1 + 1.62 r)
 *       Tn = T - F / F';   T = Tn < cap ? Tn : cap,   with lh = log(p_k / 1222.42), cap = (32.19 lh - 4780.84632) / (lh - 17.502):
 *     the temperature at which es is half of p_k.  H is increasing and convex in T, so the first step from the colder Td overshoots
 *     and the others come down; the cap keeps an overshoot where es < p_k, far above every root.  After the last step r = r(T).
 *     Every level is solved from ln theta_e and p_k alone: no level depends on the one below it.
 *   Buoyancy.  Tv(T, r) = (T (1 + r / eps)) / (1 + r);  b_k = Rd (Tv(parcel) - Tv(t[k], q[k] / (1 - q[k])));  b_s = +0.0.
 *   Areas.    Step j, kt <= j < s, lies between the levels j + 1 (lo = b_{j+1}) and j (hi = b_j);  dl = log(p_{j+1}) - log(p_j).
 *     lo and hi of strictly opposite signs: f = lo / (lo - hi); the lower triangle ((lo f) dl) / 2 and the upper ((hi (1 - f)) dl) / 2:
 *     the positive one is pos_j, the other neg_j — the step is split at the zero of the linear b, so both areas are continuous in
 *     the inputs.  Otherwise area = ((lo + hi) / 2) dl: pos_j = area, neg_j = +0.0 where area > 0; pos_j = +0.0, neg_j = area if not.
 *   Outputs.  first = the largest j with pos_j > 0: the first step from the ground that holds a positive area.
 *     cape = the sum of pos_j.  cin = the sum of neg_j over j > first, and of neg_first where lo of that step is negative (the
 *     negative triangle lies below the positive one); cin <= 0.  No step with pos_j > 0: cape = +0.0 and cin = NaN.
 *     Both sums are BLOCKED: the steps 8 m .. 8 m + 7 (ATX_PARCEL_BLOCK, aligned to the level index) are added in DESCENDING order —
 *     from the ground up, the order in which a lane that walks the column meets them — into a block sum that starts at +0.0, the
 *     block sums in descending order into the result, which starts at +0.0; an absent term is +0.0.
 *   Not outputs.  The level of free convection and the equilibrium level jump under a perturbation of the inputs (a new positive
 *     step far below moves them by kilometres); they are not given.  Mixed-layer parcels, the ice phase and reversible ascent are out.
 *   Parity.   Unpinned against earthkit-meteo, metpy and IFS: the formulas are Bolton's, as theirs are, the moist adiabat is the
 *     pseudo-adiabat of constant theta_e (eq. 43), not an integration of a lapse rate, and IFS' cape follows parcel rules of its own.
 *
 * Accuracy.  b_k is a difference of two virtual temperatures of about 300 K, so the areas carry the roundings of the logarithms
 * and of the Newton residual magnified by Tv / |Tv(parcel) - Tv(env)|.  tests/test_parcel_host.py pins numpy's own worst distance
 * from the statement in 240-bit arithmetic per case — in ulps of S = sum (pos_j - neg_j) for cape and cin, of |y| for the others —
 * and the kernels are held to twice that plus 2 ulps (float32: 0.5 ulp of the store plus that bound times 2^-29).  pstart is a copy.
 * The kernels' log and exp are the library's own, within 0.54 and 0.61 ulp (csrc/parcel/atx_parcel_math.hpp): a logarithm of 1 ulp
 * did not keep every case inside that rule.
 *
 *   t, q      n_lev rows each, n_pts points, the same layout and type; each with its own pitch
 *   sp        [n_pts] in the stack's type
 *   out       ATX_PARCEL_OUTPUTS rows, n_pts points, the layout and type of t
 *   A, B      float64 [n_lev + 1] (ATX_PARCEL_HYBRID; levels_pa is ignored)
 *   levels_pa float64 [n_lev], strictly increasing (ATX_PARCEL_PRESSURE; A and B are ignored).  Device memory: its order is the
 *             caller's to keep
 *   depth_pa, top_pa   depth and p_top in Pa (depth_pa is ignored by ATX_PARCEL_LOWEST)
 *   t_pitch, q_pitch, out_pitch   in elements: between points (ATX_COLUMNS: >= n_lev, >= ATX_PARCEL_OUTPUTS) or between rows
 *             (ATX_FIELDS: >= n_pts)
 * Both layouts and all pitches give the same bits.  ATX_COLUMNS: a 256-lane workgroup per tile of consecutive points stages their
 * columns in LDS (16-byte vectors where base and pitch allow, reads never beyond a pitch), then one lane per (point, level) for the
 * pressures and the Newton solves, a wave or a part of one per point for the start level and the first positive step, one lane per
 * (point, block) for the sums; each point's outputs leave as one contiguous run.  atx_parcel_tile_points gives the points of a
 * tile.  ATX_FIELDS: one lane per point, rows read coalesced, the scan state in registers.
 *
 * Validation comes before anything touches HIP.  ATX_EINVAL: an unknown dtype, layout, mode or parcel; n_pts < 0, n_lev < 1; a
 * top_pa that is not >= 0 or a depth_pa that is not >= 0 (NaN included); a NULL pointer for a buffer that is not empty; an out that
 * overlaps t, q or sp.  ATX_ESHAPE: a pitch too small for the shape.  ATX_ENOTIMPL: n_lev beyond ATX_PARCEL_MAX_LEVELS, n_pts beyond
 * int32, or (ATX_COLUMNS) one point beyond the LDS of a workgroup — never a silently wrong result.  No points: ATX_OK, nothing is
 * launched.
 */
typedef enum { ATX_PARCEL_HYBRID = 0, ATX_PARCEL_PRESSURE = 1 } atx_parcel_mode;
typedef enum { ATX_PARCEL_LOWEST = 0, ATX_PARCEL_MOST_UNSTABLE = 1 } atx_parcel_start;
ATX_PARCEL_API int atx_parcel_columns(const void* t, const void* q, const void* sp, void* out, const double* A, const double* B,
                                      const double* levels_pa, int64_t n_pts, int64_t n_lev, int64_t t_pitch, int64_t q_pitch, int64_t out_pitch,
                                      double depth_pa, double top_pa, int dtype, int layout, int mode, int parcel, void* stream);

/* The points of a tile of the ATX_COLUMNS kernel for this shape — what the LDS of a workgroup holds; it does not depend on the
 * pitches.  0: one point does not fit (the call is ATX_ENOTIMPL), or an argument is out of range. */
ATX_PARCEL_API int atx_parcel_tile_points(int64_t n_lev, int dtype, int mode, int parcel);

/* The kernels' own log (which = 0, positive normal x) and exp (which = 1, |x| < 700) evaluated ON THE HOST from the same source
 * (csrc/parcel/atx_parcel_math.hpp): x and y are HOST arrays of n float64.  tests/test_parcel_host.py holds them to 0.55 and 0.62 ulp
 * of 240-bit arithmetic with it.  ATX_EINVAL: an unknown `which`, a NULL pointer with n > 0, n < 0. */
ATX_PARCEL_API int atx_parcel_host_math(const double* x, double* y, int64_t n, int which);

#ifdef __cplusplus
}
#endif

#endif /* ATX_PARCEL_H */
