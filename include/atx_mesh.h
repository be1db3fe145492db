/*
 * atx_mesh.h — C ABI of libatx_mesh, the point-location kernel that goes with libatx (MI355X, gfx950).
 *
 * A companion library with its own header, as libatx_text and libatx_plan are: libatx APPLIES a regrid
 * operator, libatx_plan BUILDS one between row-structured grids, this library LOCATES target points in a
 * triangulated source grid so that a 3-point linear operator can be built from any set of source points.
 * The libraries share no symbol and no state; this header includes atx.h only for the status codes
 * (ATX_OK, ATX_EINVAL, ATX_EHIP, ...), which mean here what they mean there.
 *
 * Conventions (atx.h states them in full; they hold unchanged)
 *  - Plain C types only.  Every pointer named in a signature is a DEVICE pointer
 *    (HBM).  The caller owns every buffer; the library allocates nothing and
 *    keeps no state besides a thread-local error string.  A buffer of ZERO
 *    elements may be NULL: the call validates the rest, launches nothing and
 *    returns ATX_OK.
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls
 *    enqueue work and return without synchronising.
 *  - Return value: ATX_OK (0) or a negative ATX_E* code; atx_mesh_last_error()
 *    gives the message for the calling thread.  Nothing throws across the ABI.
 *  - Every entry point is re-entrant.
 *
 * A *mesh* is a triangulation of n_src points on the unit sphere (interp.triangulate_sphere builds it on the host with Qhull):
 *   src_xyz  double  [n_src, 3]  unit vectors, row-major
 *   tri      int32   [n_tri, 3]  vertex numbers, every triangle oriented so that det(v0, v1, v2) > 0
 *   nbr      int32   [n_tri, 3]  nbr[t, e] is the triangle across the edge opposite vertex e
 *   flag     uint8   [n_tri]     non-zero: the triangle is not part of the domain (a sliver, or an edge longer than the caller allows)
 * The library cannot read HBM on the host, so it checks sizes and pointers only; its kernel never indexes outside the arrays as
 * sized here whatever they hold.
 */
#ifndef ATX_MESH_H
#define ATX_MESH_H

#include <stddef.h>
#include <stdint.h>

#include "atx.h"

/* Built with -fvisibility=hidden and a version script made from this header: the ATX_MESH_API declarations below are the library's
 * ONLY dynamic symbols (tests/test_linear_unstructured_host.py checks `nm -D --defined-only` against this header). */
#if defined(_WIN32)
#define ATX_MESH_API
#else
#define ATX_MESH_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define ATX_MESH_VERSION 420 /* goes with ATX_VERSION */
#define ATX_MESH_MAX_STEPS 1048576 /* the largest max_steps atx_mesh_locate accepts */

/* ATX_MESH_VERSION of the library that was loaded. */
ATX_MESH_API int atx_mesh_version(void);

/* The message of the last failed call of the calling thread ("" if none); valid until that thread's next failing call. */
ATX_MESH_API const char* atx_mesh_last_error(void);

/*
 * Walk every target from its seed triangle to the triangle under it (interp.locate_walk_host states the loop; the outputs equal
 * that statement bit for bit).  One target per lane.  With
 *   det(p, b, c) = p.x (b.y c.z - b.z c.y) + p.y (b.z c.x - b.x c.z) + p.z (b.x c.y - b.y c.x)
 * every operation rounded on its own and the sum taken left to right, at triangle t = (a, b, c) and target p:
 *   1. flag[t] set: status 2 (outside), stop.
 *   2. d0 = det(p, b, c), d1 = det(p, c, a), d2 = det(p, a, b), D = det(a, b, c).
 *   3. every d_i >= -2^-30 D: status 0 (found); negative d_i become 0 and w_i = d_i / ((d0 + d1) + d2).
 *   4. max_steps moves made already: status 1 (undecided), stop.
 *   5. move to nbr[t, e], e the first of the smallest d_i.
 * A seed or neighbour outside [0, n_tri), or a vertex outside [0, n_src), ends the lane with status 3.
 *
 *   tri_out  int32  [n_tgt]     the triangle at which the lane stopped; -1 with status 3
 *   w        double [n_tgt, 3]  the weights of tri[tri_out]'s vertices with status 0; 0 with status 1 and 2; NaN with status 3
 *   status   int32  [n_tgt]     0 found, 1 undecided, 2 outside, 3 malformed mesh or seed
 *   steps    int32  [n_tgt]     moves made
 *
 * ATX_EINVAL: n_src or n_tri outside 1 .. 2^31 - 1, n_tgt outside 0 .. 2^31 - 1, max_steps outside 0 .. ATX_MESH_MAX_STEPS, or a
 * NULL pointer with n_tgt > 0 — nothing is launched.  n_tgt == 0: ATX_OK, nothing launched, the pointers may be NULL.
 */
ATX_MESH_API int atx_mesh_locate(const double* src_xyz, int64_t n_src, const int32_t* tri, const int32_t* nbr, const uint8_t* flag,
                                 int64_t n_tri, const double* tgt_xyz, const int32_t* seed, int64_t n_tgt, int32_t max_steps,
                                 int32_t* tri_out, double* w, int32_t* status, int32_t* steps, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* ATX_MESH_H */
