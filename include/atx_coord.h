/*
 * atx_coord.h — C ABI of libatx_coord, the vertical interpolation on a coordinate FIELD that goes with libatx (MI355X, gfx950): the
 * variables of a stack of levels onto surfaces of a second stack's values — pressure levels to height levels (z on pl as the
 * coordinate), pressure or model levels to surfaces of any monotone param (pt, archived z on ml).  The per-point coordinate column is
 * read from memory; libatx_levels, libatx_heights and libatx_pltz derive theirs from sp and an A / B table.
 *
 * A companion library with its own header, as libatx_text, libatx_plan, libatx_mesh, libatx_missing, libatx_stat, libatx_levels,
 * libatx_geopotential, libatx_heights and libatx_pltz are: libatx's entry points are a fixed, tested set (include/atx.h, ATX_VERSION
 * 420).  The libraries share no symbol and no state; this header includes atx.h for the status codes, atx_dtype and atx_layout, which
 * mean here what they mean there.
 *
 * Conventions (atx.h states them in full; they hold unchanged)
 *  - Plain C types only.  Every pointer named in a signature is a DEVICE pointer (HBM).  The caller owns every buffer; the library
 *    keeps no state besides a thread-local error string.  A buffer of ZERO elements may be NULL.
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls enqueue work and return without synchronising.
 *  - Return value: ATX_OK (0) or a negative ATX_E* code; atx_coord_last_error() gives the message for the calling thread.
 *  - Every entry point is re-entrant.
 */
#ifndef ATX_COORD_H
#define ATX_COORD_H

#include <stddef.h>
#include <stdint.h>

#include "atx.h"

/* Built with -fvisibility=hidden and a version script made from this header: the ATX_COORD_API declarations below are the
 * library's ONLY dynamic symbols (tests/test_host_api.py checks `nm -D --defined-only` against this header). */
#if defined(_WIN32)
#define ATX_COORD_API
#else
#define ATX_COORD_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define ATX_COORD_VERSION 420 /* goes with ATX_VERSION */

#define ATX_COORD_MAX_LEVELS 256 /* rows per variable that one call takes; more is ATX_ENOTIMPL */

/* The accuracy of an interior result against the statement in exact arithmetic on the same inputs, in float64 ulps of
 * max(|x[a]|, |x[b]|) (the derivation is below).  A float32 stack adds its one rounding at the store: 0.5 + 11 * 2^-29 float32 ulps. */
#define ATX_COORD_ULPS_F64 11

/* ATX_COORD_VERSION of the library that was loaded. */
ATX_COORD_API int atx_coord_version(void);

/* The message of the last failed call of the calling thread ("" if none); valid until that thread's next failing call. */
ATX_COORD_API const char* atx_coord_last_error(void);

/*
 * Interpolation on a coordinate field.  For one grid point p: the n = n_lev rows c[0..n-1] of the coordinate column, the rows
 * x[0..n-1] of a variable's column on the same levels, and the targets.  All arithmetic is in float64 for both storage widths, one
 * operation at a time, without contraction, with IEEE divisions; the result is rounded once at the store.
 *
 *   Target.   T = targets[t] + (double)offset[p], or T = targets[t] where offset == NULL.  The rounded sum IS the target: no
 *             coordinate value is ever shifted, so no weight suffers cancellation from the offset ("above the ground": offset = zs).
 *   Usable column.   n == 1 and c[0] is not NaN;  or all n - 1 steps c[k+1] - c[k] are strictly positive;  or all are strictly
 *             negative.  Anything else — a NaN anywhere in c, an equal pair, a change of direction — is unusable: every output of
 *             the point is NaN and bad[p] = 1.  The direction is per point: ascending and descending columns may sit side by side.
 *   Bracket.  e, x: the column and a variable read in ascending order of c (reversed where c descends).  i = #{k : e[k] <= T}.
 *               0 < i < n            a = i - 1, b = i;  w = (T - e[a]) / (e[b] - e[a]);  y = x[a] + w * (x[b] - x[a])
 *               i == n, T == e[n-1]  y = x[n-1]
 *               i == n otherwise     ATX_COORD_NEAREST: y = x[n-1];  ATX_COORD_MISSING: y = NaN
 *               i == 0               ATX_COORD_NEAREST: y = x[0];    ATX_COORD_MISSING: y = NaN
 *             A NaN target (or a NaN offset) counts nothing and is handled as i == 0.
 *   Floor.    Where floor != NULL and T < (double)floor[p]: y = NaN, whatever the policy ("above the sea but under the ground": floor =
 *             zs).  A NaN floor never triggers.
 *   The bracket and w of a (point, target) pair are computed once and applied to all n_var variables.  A target exactly on a level
 *   has w == 0 and returns x[a] + 0 * (x[b] - x[a]): that level's bits for every finite bracket (+0.0 for -0.0).  A NaN in x reaches
 *   only the targets whose bracket holds it.  Which NaN is written is unspecified.
 *   Scope.    Only the LINEAR coordinate: an interpolation in the logarithm of the coordinate (pressure as the coordinate field) is
 *             not part of this statement — hand the library log(c) and log targets computed elsewhere, or use libatx_levels.
 *   Parity.   earthkit-meteo's interpolation on a monotone coordinate is the same family; parity is unpinned.
 *
 * Accuracy (ATX_COORD_ULPS_F64).  With u = 2^-53 and every operation rounded once: N = T - e[a] in [0, D), D = e[b] - e[a] > 0,
 * fl(N) = N (1 + e1), fl(D) = D (1 + e2), w = fl(N) / fl(D) (1 + e3), fl(x[b] - x[a]) = (x[b] - x[a]) (1 + e4),
 * s = w fl(x[b] - x[a]) (1 + e5) = (N / D) (x[b] - x[a]) (1 + theta) with |theta| <= 5 u + O(u^2), and y = (x[a] + s) (1 + e6): six
 * roundings.  The exact y* = x[a] + (N / D) (x[b] - x[a]) lies between x[a] and x[b], so with M = max(|x[a]|, |x[b]|): |y*| <= M and
 * |(N / D) (x[b] - x[a])| <= 2 M, hence |y - y*| <= 5 u 2 M + u M + O(u^2) = 11 u M, and u M is less than one ulp of M.  The bound
 * supposes that no intermediate overflows or is subnormal.
 *
 *   src     n_var variables x n_lev rows each, variables adjacent (rows v * n_lev .. v * n_lev + n_lev - 1 are variable v), n_pts points
 *   coord   n_lev rows: the coordinate of every row at every point, in the layout and type of src
 *   out     n_var x n_tgt rows (row v * n_tgt + t is variable v at targets[t]), n_pts points, the layout and type of src
 *   offset  [n_pts] in the stack's type, or NULL (0: T = targets[t])
 *   floor   [n_pts] in the stack's type, or NULL
 *   bad     uint8 [n_pts] or NULL: written for every point by the launch, 1 where the coordinate column is unusable, else 0 (plain
 *           vector stores, no atomics)
 *   targets float64 [n_tgt]: any order, duplicates allowed, the output is in the given order
 *   src_pitch, coord_pitch, out_pitch   in elements: between points (ATX_COLUMNS: >= n_var * n_lev, >= n_lev, >= n_var * n_tgt) or
 *           between rows (ATX_FIELDS: >= n_pts)
 * Both layouts give the same bits.  ATX_COLUMNS: a workgroup stages the coordinate columns and the variable columns of a run of
 * consecutive points in LDS with loads that cover the run contiguously — each of the two stacks on its own route: 16-byte vectors
 * where its base is 16-byte aligned, its pitch a multiple of 16 bytes and the last vector of a column inside the pitch (reads may
 * cover the pitch padding inside that vector, nothing beyond), single elements otherwise; both routes give the same bits — and writes
 * each point's outputs as one contiguous run.  ATX_FIELDS: one lane per (point, target), the coordinate rows read strided.
 *
 * Validation comes before anything touches HIP.  ATX_EINVAL: an unknown dtype, layout or policy; n_pts < 0, n_var < 1, n_lev < 1,
 * n_tgt < 0; a NULL pointer for a buffer that is not empty; an out or a bad that overlaps src, coord, offset or floor, or each
 * other.  ATX_ESHAPE: a pitch too small for the shape.  ATX_ENOTIMPL: n_lev > ATX_COORD_MAX_LEVELS, sizes beyond int32, or
 * (ATX_COLUMNS) one point's columns and outputs beyond the LDS of a workgroup — never a silently wrong result.  No points or no
 * targets: ATX_OK, nothing is launched (and bad is not written).
 */
typedef enum { ATX_COORD_NEAREST = 0, ATX_COORD_MISSING = 1 } atx_coord_outside;
ATX_COORD_API int atx_coord_interpolate(const void* src, const void* coord, void* out, const void* offset, const void* floor, uint8_t* bad,
                                        const double* targets, int64_t n_pts, int64_t n_var, int64_t n_lev, int64_t n_tgt, int64_t src_pitch,
                                        int64_t coord_pitch, int64_t out_pitch, int dtype, int layout, int outside, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* ATX_COORD_H */
