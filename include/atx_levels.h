/*
 * atx_levels.h — C ABI of libatx_levels, the vertical interpolation that goes with libatx (MI355X, gfx950): the model levels of a
 * stack of variables to pressure levels, one column at a time.
 *
 * A companion library with its own header, as libatx_text, libatx_plan, libatx_mesh, libatx_missing and libatx_stat are: libatx's
 * entry points are a fixed, tested set (include/atx.h, ATX_VERSION 420).  The libraries share no symbol and no state; this header
 * includes atx.h for the status codes, atx_dtype and atx_layout, which mean here what they mean there.
 *
 * Conventions (atx.h states them in full; they hold unchanged, with ONE exception named below)
 *  - Plain C types only.  Every pointer named in a signature is a DEVICE pointer (HBM) — except `level_index`, which is a HOST
 *    pointer: the library reads it during the call, checks it, and hands it to the kernel by value.  The caller owns every buffer; the
 *    library keeps no state besides a thread-local error string.  A buffer of ZERO elements may be NULL.
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls enqueue work and return without synchronising.
 *  - Return value: ATX_OK (0) or a negative ATX_E* code; atx_levels_last_error() gives the message for the calling thread.
 *  - Every entry point is re-entrant.
 */
#ifndef ATX_LEVELS_H
#define ATX_LEVELS_H

#include <stddef.h>
#include <stdint.h>

#include "atx.h"

/* Built with -fvisibility=hidden and a version script made from this header: the ATX_LEVELS_API declarations below are the
 * library's ONLY dynamic symbols (tests/test_host_api.py checks `nm -D --defined-only` against this header). */
#if defined(_WIN32)
#define ATX_LEVELS_API
#else
#define ATX_LEVELS_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define ATX_LEVELS_VERSION 420 /* goes with ATX_VERSION */

#define ATX_LEVELS_MAX_LEVELS 256 /* rows per variable that one call takes; more is ATX_ENOTIMPL */

/* ATX_LEVELS_VERSION of the library that was loaded. */
ATX_LEVELS_API int atx_levels_version(void);

/* The message of the last failed call of the calling thread ("" if none); valid until that thread's next failing call. */
ATX_LEVELS_API const char* atx_levels_last_error(void);

/*
 * Model levels to pressure levels.  For one grid point: the surface pressure sp, the half-level coefficients A[0..H-1], B[0..H-1]
 * (H = n_half = model levels + 1), the n = n_lev rows x[0..n-1] of a variable's column, top first, and each row's 0-based model level
 * m[k] = level_index[k] (k itself where level_index == NULL), strictly increasing: 0..n-1 when the whole model is present, a subset
 * such as levels 60-137 otherwise.  All arithmetic is in float64 for both storage widths, statement by statement, without contraction,
 * with IEEE divisions; the result is rounded once at the store:
 *     p_half(j) = A[j] + B[j] * sp
 *     p_full[k] = (p_half(m[k]) + p_half(m[k] + 1)) / 2
 *     p_ground  = p_half(H - 1)
 *     c(p)      = p  (ATX_LEVELS_LINEAR)   or   log(p)  (ATX_LEVELS_LOG; the library's own logarithm, <= 1 ulp)
 * For a target pressure P (Pa):  i = #{k : p_full[k] <= P}, counted over the WHOLE column.
 *     sp != sp            y = NaN, whatever the policy (every comparison fails: i = 0)
 *     0 < i < n           a = i - 1, b = i;  w = (c(P) - c(p_full[a])) / (c(p_full[b]) - c(p_full[a]));  y = x[a] + w * (x[b] - x[a])
 *     i == n, P <= p_ground   (the half layer between the lowest full level and the ground)   y = x[n - 1]
 *     i == n, P >  p_ground   (below the ground: `!(P <= p_ground)`)   ATX_LEVELS_NEAREST: y = x[n - 1];  ATX_LEVELS_MISSING: y = NaN
 *     i == 0                  (above the top full level)               ATX_LEVELS_NEAREST: y = x[0];      ATX_LEVELS_MISSING: y = NaN
 * So: a target exactly on a full level has w == 0 and returns that level's value (x[a] + 0 * (x[b] - x[a]): its bits for every finite
 * bracket, +0.0 for -0.0); a NaN in x reaches only the targets whose bracket holds it; n == 1 has no interior; a NaN target counts
 * nothing and is "above the top".  Which NaN is written is unspecified.  The t / z extrapolations of IFS below the ground and height
 * level targets are not part of this statement.  earthkit-meteo's and MARS' interpolations are the same family; parity is unpinned.
 *
 *   src   n_var variables x n_lev rows each, variables adjacent (rows v * n_lev .. v * n_lev + n_lev - 1 are variable v), n_pts points
 *   out   n_var x n_tgt rows (row v * n_tgt + t is variable v at targets[t]), n_pts points, the layout and type of src
 *   sp    [n_pts], the stack's type;  A, B  float64 [n_half];  targets  float64 [n_tgt] in Pa: any order, duplicates allowed, the
 *         output is in the given order;  level_index  HOST int32 [n_lev] or NULL
 *   src_pitch, out_pitch   in elements: between points (ATX_COLUMNS: >= n_var * n_lev, >= n_var * n_tgt) or between rows (ATX_FIELDS:
 *         >= n_pts).  The bracket and the weight of a (point, target) pair are computed once and applied to all n_var variables.
 * Both layouts give the same bits.  ATX_COLUMNS: a workgroup stages the columns of a run of consecutive points in LDS with loads that
 * cover the run contiguously — 16-byte vectors where src is 16-byte aligned, src_pitch a multiple of 16 bytes and the last vector of a
 * column inside the pitch (reads may cover the pitch padding inside that vector, nothing beyond), single elements otherwise — and
 * writes each point's outputs as one contiguous run.  ATX_FIELDS: one lane per (point, target).
 *
 * Validation comes before anything touches HIP.  ATX_EINVAL: an unknown dtype, layout, coordinate or policy; n_pts < 0, n_var < 1,
 * n_lev < 1, n_tgt < 0, n_half < 2; a level_index that is not strictly increasing inside 0 .. n_half - 2 (NULL: n_lev > n_half - 1);
 * a NULL pointer for a buffer that is not empty.  ATX_ESHAPE: a pitch too small for the shape.  ATX_ENOTIMPL: n_lev >
 * ATX_LEVELS_MAX_LEVELS, sizes beyond int32, or (ATX_COLUMNS) one point's columns, pressures and brackets beyond the LDS of a
 * workgroup — never a silently wrong result.  No points or no targets: ATX_OK, nothing is launched.
 */
typedef enum { ATX_LEVELS_LINEAR = 0, ATX_LEVELS_LOG = 1 } atx_levels_coordinate;
typedef enum { ATX_LEVELS_NEAREST = 0, ATX_LEVELS_MISSING = 1 } atx_levels_outside;
ATX_LEVELS_API int atx_levels_interpolate(const void* src, void* out, const void* sp, const double* A, const double* B,
                                          const int32_t* level_index, const double* targets, int64_t n_pts, int64_t n_var, int64_t n_lev,
                                          int64_t n_tgt, int64_t n_half, int64_t src_pitch, int64_t out_pitch, int dtype, int layout,
                                          int coordinate, int outside, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* ATX_LEVELS_H */
