/*
 * atx.h — C ABI of libatx, the MI355X (gfx950) field-transform kernels.
 *
 * This is the drop-in boundary for the filter hot path of ecmwf/anemoi-transform
 * 0.4.2.  The reference is pure Python and has NO native interface on this
 * path: its filters call numpy / scipy in-process.  Every entry point below
 * therefore replaces a numpy/scipy *statement* of the reference, cited as
 * `R:` (paths relative to /root/reference/src/anemoi/transform/).  The
 * reference-side binding a maintainer would add (a ctypes stub) is shown in
 * INTEGRATION.md.
 *
 * Conventions
 *  - Plain C types only.  Every pointer named in a signature is a DEVICE
 *    pointer (HBM) unless the comment says "host".  The caller owns every
 *    buffer; the library allocates nothing and keeps no state besides a
 *    thread-local error string.  A buffer of ZERO elements — a stack of no
 *    points, the output of a regrid to no targets — may have no storage: its
 *    pointer may be NULL, the call validates the rest, does nothing and
 *    returns ATX_OK (allocators hand out NULL for empty tensors).
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).
 *    Calls enqueue work and return without synchronising.
 *  - Return value: ATX_OK (0) or a negative ATX_E* code; atx_last_error()
 *    gives the message for the calling thread.  Nothing throws across the ABI.
 *  - Threading: every entry point is re-entrant.  The library holds no state
 *    between calls besides two PER-THREAD items — the error string and the
 *    tuning hook (atx_set_tuning) — and the RCCL binding, resolved once under
 *    std::call_once.  Several host threads may call at the same time, each on
 *    its own stream and buffers (or one thread may drive several streams); a
 *    call that fails in one thread leaves the other threads' atx_last_error()
 *    untouched.  Two calls that write the same buffer, or share a `workspace`,
 *    must be ordered by the caller (same stream, or an event).
 *    tests/test_gpu_threads.py: 4 threads x 6 rounds of atx_regrid_ell (direct
 *    and, through the per-thread tuning hook, tiled), atx_pointwise_stack,
 *    atx_reduce_stack and atx_mask_build + atx_mask_to_index at once, every
 *    result against the CPU oracle, one thread provoking ATX_EINVAL.
 *  - A *stack* is a batch of `n_lev` fields on one grid of `n_pts` points.
 *    Two HBM layouts (atx_layout):
 *      ATX_COLUMNS  element (point p, level l) at  base[p * pitch + l]
 *                   — all levels of one grid point are contiguous (a model
 *                   column).  The engine's native layout: a neighbour read is
 *                   one contiguous n_lev*B-byte run.
 *      ATX_FIELDS   element (p, l) at base[l * pitch + p] — one field after
 *                   the other, the reference's unit (`field.to_numpy()`).
 *    `pitch` is in ELEMENTS (>= n_lev for ATX_COLUMNS, >= n_pts for ATX_FIELDS).
 *  - dtype: ATX_F32 or ATX_F64; weights / scalars use the data dtype
 *    (double parameters are rounded to float for ATX_F32, as numpy does for a
 *    python-float operand).
 *  - Floating point is evaluated WITHOUT contraction (no FMA): x*a+b is two
 *    roundings, a CSR row is summed sequentially from 0 in index order, so the
 *    f64 results are bit-identical to numpy / scipy.
 */
#ifndef ATX_H
#define ATX_H

#include <stddef.h>
#include <stdint.h>

/* The library is built with -fvisibility=hidden: the ATX_API declarations below are its ONLY dynamic symbols
 * (tests/test_host_api.py checks `nm -D --defined-only` against this header), so nothing of its C++ internals can
 * interpose, or be interposed by, another library of the process (torch's own HIP libraries, RCCL). */
#if defined(_WIN32)
#define ATX_API
#else
#define ATX_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define ATX_VERSION 420 /* 0.4.2 — additions only, so the number stays: atx_obs_row_expr / atx_obs_keep_positions (a postfix row-expression
                           * program with its atx_expr_op codes, keep bits and their row positions; for one commit, under this number
                           * only and with the Python binding as their single caller, they were reached through atx_obs_column_ops codes
                           * 64 .. 99, which are unknown codes again); a second family of atx_obs_column_ops codes, ATX_COLOP_SCALAR ..
                           * ATX_COLOP_FILL_NAN (the compares, selects and row predicates of the tabular QC filters; no new entry point); atx_obs_order_key / atx_obs_mark_first / atx_obs_take_rows (row
                           * sets: pandas' order and equality as int64 keys, first occurrences, a gather of rows) with the
                           * atx_key_dtype enum; atx_obs_column_ops (a program of library functions over
                           * columns) with its ATX_COLOP_* codes; atx_obs_fill_heights (missing station altitudes from an
                           * orography); atx_healpix_ang2pix (HEALPix pixel indices per row) with its atx_healpix_scheme enum; atx_obs_forcings / atx_obs_view_angles / atx_obs_planck_bt (per-row
                           * observation operators); atx_obs_group_mean / atx_obs_group_argmin (superob: per-group
                           * means by pandas' row-order Kahan rule and the nearest row of every group); atx_obs_best_per_cell / atx_obs_fill_stack (observation tables
                           * onto a grid: a keyed arg-min and the gather that fills the stack); atx_rotate_vectors_stack (vector components between projection
                           * frames, a per-point table shared by every level) with its atx_frame enum; atx_pressure_at_height_stack (the
                           * first vertical reduction, one value per model column) and two multi-input operators, ATX_COMB_Q_TO_D /
                           * ATX_COMB_D_TO_Q; no existing signature, enum value or layout changed.
                           * round 6: nothing changed but two relaxations — the declarations carry ATX_API (the library exports nothing else),
                           * and zero-element buffers may be NULL (see Conventions).
                           * round 5: no signature, enum or layout changed.  The float64 library functions are the library's own routines now
                           * (ATX_OP_EXP, ATX_OP_LOG, the tanh of ATX_COMB_SNOW_COVER, the polynomials of ATX_COMB_COS_SIN): results may differ from 0.4.1 in the
                           * last bit and stay within 1 ulp (exp, log), 2 ulp (cos, sin) and 4 ulp (tanh) of numpy's, as before.
                           * 0.4.1 — eight more multi-input operators (ATX_COMB_OPERA_CLIP .. ATX_COMB_R_TO_Q); nothing else changed.
                           * 0.4.0 — round 4: atx_vector_program takes the CAPACITY of `out` (ATX_EWORKSPACE when too small — 0.3 wrote its
                           * grown table without asking), atx_reduce* keep the no-atomics route for every shape when given a workspace.
                           * 0.3.0 — round 3: atx_reduce* take a workspace, atx_regrid_*_ordered, two more multi-input operators, and the
                           * table written by atx_vector_program grew a typed per-level part (a table built by a 0.2 library is too short for
                           * 0.3+ kernels: check atx_version() >= 300 before passing one as vec_prog) */

/* ---- status codes --------------------------------------------------------- */
enum {
    ATX_OK = 0,
    ATX_EINVAL = -1,   /* bad argument (null pointer, negative size, bad enum) -> ValueError */
    ATX_ESHAPE = -2,   /* inconsistent shapes / pitches -> AssertionError (R: filters/fields/regrid.py:377-378) */
    ATX_ENOTIMPL = -3, /* unsupported combination -> NotImplementedError (R: regrid.py:332-335) */
    ATX_EHIP = -4,     /* HIP runtime error at launch */
    ATX_EALIGN = -5,   /* pointer / pitch alignment not met for the requested layout */
    ATX_EWORKSPACE = -6, /* workspace too small */
    ATX_ECOMM = -7      /* RCCL missing or a collective failed */
};

typedef enum { ATX_F32 = 0, ATX_F64 = 1 } atx_dtype;
typedef enum { ATX_COLUMNS = 0, ATX_FIELDS = 1 } atx_layout;

/* comparison operators of apply_mask (R: filters/fields/apply_mask.py:23-36:
 * the 12 spellings map onto these 6) plus the NaN test of remove_nans
 * (R: filters/fields/remove_nans.py:101  `~np.isnan(data)`). */
typedef enum {
    ATX_CMP_GT = 0,
    ATX_CMP_LT = 1,
    ATX_CMP_EQ = 2,
    ATX_CMP_NE = 3,
    ATX_CMP_GE = 4,
    ATX_CMP_LE = 5,
    ATX_CMP_NOTNAN = 6, /* threshold ignored */
    ATX_CMP_ISNAN = 7   /* threshold ignored */
} atx_cmp;

/* per-point operators (one per reference statement). p0/p1 are the scalars. */
typedef enum {
    ATX_OP_COPY = 0,       /* y = x (bit copy)                                               */
    ATX_OP_AFFINE = 1,     /* y = x*p0 + p1        R: filters/fields/rescale.py:25           */
    ATX_OP_AFFINE_INV = 2, /* y = (x - p1) / p0    R: rescale.py:28                          */
    ATX_OP_MUL = 3,        /* y = x * p0           R: filters/fields/orog_to_z.py:59         */
    ATX_OP_DIV = 4,        /* y = x / p0           R: orog_to_z.py:77 (a true division)      */
    ATX_OP_CLIP = 5,       /* y = np.clip(x,p0,p1) R: filters/fields/clipper.py:69; a NaN
                              bound means "no bound on that side"; NaN x stays NaN          */
    ATX_OP_IMPUTE_NAN = 6, /* y = isnan(x)?p0:x    R: filters/fields/impute_nans.py:53-54    */
    ATX_OP_EXP = 7,        /* y = exp(x)           R: filters/fields/lnsp_to_sp.py:47        */
    ATX_OP_LOG = 8,        /* y = log(x)           R: lnsp_to_sp.py:65                       */
    ATX_OP_SET_NAN = 9,    /* y = NaN (canonical quiet NaN)                                  */
    ATX_OP_COUNT_ = 10
} atx_op;

/* One step of a per-level program: level l of a stack is transformed by
 * prog[s * n_lev + l] for s = 0 .. n_stage-1 in turn.  ATX_OP_COPY leaves the
 * level untouched (bit-exact pass-through of unselected fields,
 * R: filter.py:193-194).  `use_mask` != 0 additionally writes NaN where the
 * point mask is set, AFTER the arithmetic of that stage
 * (R: apply_mask.py:185 `values[self.mask] = np.nan`). */
typedef struct {
    int32_t op;       /* atx_op */
    int32_t use_mask; /* 0/1 */
    double p0;
    double p1;
} atx_level_op;

/* ---- library ------------------------------------------------------------- */
ATX_API int atx_version(void);
ATX_API const char* atx_last_error(void);          /* host string, valid until the next failing call of this thread */
ATX_API const char* atx_strerror(int code);        /* host string, static */
/* DIAGNOSTIC, not part of the numerical contract: the launch form the calling thread's last atx_pointwise_stack took — "sparse",
 * "uniform", "runs", "table", "typed", "levels", "flat", "row_chunk", "row_chunk_scalar" (column stacks), "fields", "fields_scalar"
 * (field-major stacks) — or "none" when that call returned before any launch (no points, an in-place program with nothing to do, an
 * argument error) and before the first call.  After a program that was run in two halves (per-level tables beyond the LDS) it names
 * the second half's.  Which form serves which call may change between versions; results never depend on it.  Host string, static. */
ATX_API const char* atx_last_route(void);
/* DIAGNOSTIC, a second cell beside atx_last_route: the launch form the calling thread's last gather (atx_regrid_ell / _batch /
 * _ordered, atx_regrid_csr / _ordered) took, nine fields joined by '/':
 *   table      cols_ell | cols_csr | fields_ell | fields_csr              (layout and table)
 *   kernel     direct | tiled (column stacks); lanes (fields_ell); head4 | head8 | long (fields_csr)
 *   epilogue   none | uniform | runs | table (direct); none | lds (tiled, cols_csr); none | global (field-major); split when the
 *              fused program did not fit beside the tile: the plain gather ran and atx_pointwise_stack finished the program in
 *              place (atx_last_route then names the per-point form that did)
 *   width      vec | scalar (column stacks: 16-byte vectors or single elements); lane (field-major)
 *   k<K>       the compile-time k as instantiated, k0 for a runtime loop (the tiled kernel folds k > 4 to 0, padded tables start
 *              at 3, CSR rows are always k0)
 *   padded | plain        ATX_ELL_PADDED
 *   weighted | pure       pure: the k = 1 gather without weights
 *   range | stripe        how workgroups are dealt to the XCDs
 *   ordered | natural     whether tgt_rows was given
 * e.g. "cols_ell/direct/uniform/vec/k4/plain/weighted/range/natural".  "none" before the first call and after a call that launched
 * nothing (n_tgt == 0, an argument error).  Of a batch cut into several launches it names the last.  Spelling and choice may change
 * between versions; results never depend on it.  Host string, valid until the calling thread's next read. */
ATX_API const char* atx_last_gather_route(void);
/* Number of HIP devices visible, or a negative ATX_EHIP. */
ATX_API int atx_device_count(void);
/* Tuning hook for benchmarks and tests: tile > 0 runs the ATX_COLUMNS regrid through the TILED kernels with that
 * many targets per workgroup; 0 = built-in choice (the direct kernel where it applies, else the tile heuristic).
 * Per CALLING THREAD (thread-local since round 3: the launches of other threads are not affected); results never depend on it,
 * only speed. */
ATX_API int atx_set_tuning(int tile);

/* ---- regrid: precomputed index(+weight) gather ---------------------------- */

/*
 * Fixed-k ("ELL") interpolation:  out[t, l] = sum_{j<k} w[t*k+j] * src[idx[t*k+j], l]
 * accumulated from 0 in j order.
 *   w == NULL : pure gather, k must be 1:  out[t, l] = src[idx[t], l]  (bit copy)
 *     R: regrid.py:380  `data = data[..., self.nearest_grid_points]`
 *     R: regrid.py:420  `data = data[..., self.mask]` (integer / compressed boolean mask)
 *     R: filters/fields/remove_nans.py:113 `data[self._mask]` (via atx_mask_to_index)
 *   w != NULL : R: regrid.py:310 `data = self.matrix @ data` for a CSR matrix whose
 *     rows all hold k entries (k-NN weights, bilinear).
 * idx: int32 [n_tgt*k], every value in [0, n_src) (check with atx_check_indices).
 * flags: 0, or ATX_ELL_PADDED (needs weights): a NEGATIVE index marks an absent entry of a padded
 *      row and is skipped (not multiplied by zero), so ragged rows of at most k entries (e.g. MIR's
 *      3-4 entries per row) run on this kernel with exactly the CSR summation order; a row of only
 *      absent entries gives 0 as scipy does.
 * w  : dtype  [n_tgt*k].
 * prog (optional, device, n_stage*n_lev entries): per-level epilogue applied to
 *   the interpolated value before it is stored (the fused regrid -> per-point
 *   chain, R: workflows/pipeline.py:46-48 without materialising intermediates);
 *   tgt_mask (optional, uint8 [n_tgt]) is the point mask used by `use_mask`.
 *   Two optional companions of prog (NULL is always valid; results never depend on them) keep the epilogue on the
 *   fastest kernel, which has no per-workgroup set-up:
 *     host_prog (HOST)   the same n_stage*n_lev entries as prog, readable by the library: when, per stage, the levels
 *               run one operator — or one up to a level and another from there on (a stack "136 levels of t, then orog"),
 *               the change on a 16-byte boundary — the operators (<= 4 stages) are passed to the kernel by value;
 *     vec_prog  (device) atx_vector_program(prog) of the stack's dtype — the per-16-byte-vector operator table, used
 *               (together with host_prog) for programs made of COPY / AFFINE / MUL with or without the mask, <= 4 stages.
 * Requirements: ATX_COLUMNS with 16-byte aligned bases and pitches that are
 *   multiples of 16 bytes take the vector path; anything else a scalar path.
 * Layouts (MI355X, O1280 -> 0.25 deg, 137 levels, fraction of the HBM peak on algorithmic bytes): ATX_COLUMNS is the gather's
 *   layout — k = 4: 0.68-0.70, k = 16: 0.52-0.59.  ATX_FIELDS (the reference's array order) runs k <= 4 and short ragged rows at
 *   0.35-0.42, but a row of more than ~8 entries re-fetches every source point once per row that uses it (k = 16: 11.5 ms against
 *   0.93 ms): convert such stacks with atx_relayout first — both conversions included that is still 4x faster (what
 *   GatherPlan.apply does by itself).  The per-point entry points run field-major stacks at full speed (0.79-0.84).
 */
#define ATX_ELL_PADDED 1
ATX_API int atx_regrid_ell(const void* src, void* out, const int32_t* idx, const void* w,
                           int64_t n_src, int64_t n_tgt, int32_t k, int64_t n_lev,
                           int64_t src_pitch, int64_t out_pitch, int dtype, int layout, int32_t flags,
                           const atx_level_op* prog, const atx_level_op* vec_prog, const atx_level_op* host_prog,
                           int32_t n_stage, const uint8_t* tgt_mask, void* stream);

/* atx_regrid_ell applied to n_stack source stacks of identical shape, dtype and pitch with ONE launch per 16 stacks
 * (ATX_COLUMNS: grid.y = stack, no launch gaps or per-launch tails; field-major stacks are launched one after the
 * other).  srcs / outs are HOST arrays of n_stack device pointers; any n_stack >= 1.
 *   R: regrid.py:204-208 — the per-field loop, when the FieldList holds several variables / time steps on one grid
 *      pair (BASELINE config 4), or the N source stacks of a target-sharded multi-GPU step. */
ATX_API int atx_regrid_ell_batch(const void* const* srcs, void* const* outs, int32_t n_stack, const int32_t* idx, const void* w,
                                 int64_t n_src, int64_t n_tgt, int32_t k, int64_t n_lev, int64_t src_pitch, int64_t out_pitch,
                                 int dtype, int layout, int32_t flags, const atx_level_op* prog, const atx_level_op* vec_prog,
                                 const atx_level_op* host_prog, int32_t n_stage, const uint8_t* tgt_mask, void* stream);

/* The same with an ORDERED traversal of the targets: row t of idx / w is the table row of OUTPUT row tgt_rows[t] (a permutation
 * of 0 .. n_tgt-1, device int32; tgt_mask stays indexed by output row).  The result is identical to atx_regrid_ell_batch on the
 * un-permuted tables, bit for bit — only the order in which the device visits the targets changes.  Visiting a lat-lon target grid
 * in column blocks (each block top to bottom) lets vertically adjacent targets, whose neighbour patches overlap, meet in an XCD's
 * L2.  Measured on O1280 -> 0.25 degree, 137 levels (profiles/r03_column_blocks_experiment.log): k = 16 +9-12 %, k = 8 +5-9 %;
 * k <= 4 is 2-7 % SLOWER (the output rows are then written band by band) — order long rows only.  ATX_COLUMNS only. */
ATX_API int atx_regrid_ell_ordered(const void* const* srcs, void* const* outs, int32_t n_stack, const int32_t* idx, const void* w,
                                   const int32_t* tgt_rows, int64_t n_src, int64_t n_tgt, int32_t k, int64_t n_lev, int64_t src_pitch,
                                   int64_t out_pitch, int dtype, int layout, int32_t flags, const atx_level_op* prog,
                                   const atx_level_op* vec_prog, const atx_level_op* host_prog, int32_t n_stage, const uint8_t* tgt_mask,
                                   void* stream);

/*
 * General CSR interpolation: out[t, l] = sum_{jj in [indptr[t], indptr[t+1])} data[jj] * src[indices[jj], l]
 * accumulated from 0 in jj order — scipy's csr_matvec.
 *   R: regrid.py:281-285 (npz keys matrix_data f64 / matrix_indices int32 / matrix_indptr int32)
 *   R: regrid.py:310
 * indptr int32 [n_tgt+1] (device), indices int32 [nnz], data dtype [nnz].
 */
ATX_API int atx_regrid_csr(const void* src, void* out, const int32_t* indptr, const int32_t* indices,
                           const void* data, int64_t n_src, int64_t n_tgt, int64_t nnz, int64_t n_lev,
                           int64_t src_pitch, int64_t out_pitch, int dtype, int layout,
                           const atx_level_op* prog, int32_t n_stage, const uint8_t* tgt_mask,
                           void* stream);
/* atx_regrid_csr with an ORDERED traversal: CSR row t (indptr[t] .. indptr[t+1]) is the row of OUTPUT point tgt_rows[t] — see
 * atx_regrid_ell_ordered; rows of 9-16 entries gain like k = 16 there.  ATX_COLUMNS only. */
ATX_API int atx_regrid_csr_ordered(const void* src, void* out, const int32_t* indptr, const int32_t* indices, const void* data,
                                   const int32_t* tgt_rows, int64_t n_src, int64_t n_tgt, int64_t nnz, int64_t n_lev, int64_t src_pitch,
                                   int64_t out_pitch, int dtype, int layout, const atx_level_op* prog, int32_t n_stage,
                                   const uint8_t* tgt_mask, void* stream);

/* Debugging aid for binders that build their own tables: with ATX_VALIDATE=1 in the environment (read once per process) every
 * atx_regrid_* call first range-checks idx / indices / indptr / tgt_rows on the device and refuses the launch with ATX_EINVAL if an
 * entry points outside the stack (the kernels trust their tables: an out-of-range read is a GPU fault).  It synchronises the stream
 * and costs a pass over the tables; off by default. */

/* Counts entries of idx[0..n) outside [0, n_src) into *n_bad (device int64,
 * zeroed by the call).  cKDTree returns n_src for "no neighbour within
 * distance_upper_bound" (R: spatial.py:630-632) — reject before gathering. */
ATX_API int atx_check_indices(const int32_t* idx, int64_t n, int64_t n_src, int64_t* n_bad, void* stream);

/* ---- per-point transforms -------------------------------------------------- */

/*
 * y[p, l] = prog_{n_stage-1}( ... prog_0(x[p, l]) )  for every level l of a stack.
 * x == y (in place) is allowed when the pitches agree.  point_mask: uint8
 * [n_pts] or NULL (required if any stage has use_mask).
 * vec_prog (device, optional): atx_vector_program(prog) of the stack's dtype; host_prog (HOST, optional): the same
 * entries as prog, readable by the library.  With both, an IN-PLACE call whose program leaves most levels alone
 * (ATX_OP_COPY) visits only the 16-byte columns holding an active level (1 of 137 levels: 5x faster).  NULL is always
 * valid for either; results never depend on them.
 *   R: filter.py:188-196 (SingleFieldFilter map over fields), rescale.py:25,28,
 *      orog_to_z.py:59,77, clipper.py:69, impute_nans.py:53-54, lnsp_to_sp.py:47,65,
 *      apply_mask.py:183-185, glacier_mask.py:33
 */
ATX_API int atx_pointwise_stack(const void* x, void* y, int64_t n_pts, int64_t n_lev,
                                int64_t x_pitch, int64_t y_pitch, int dtype, int layout,
                                const atx_level_op* prog, const atx_level_op* vec_prog, const atx_level_op* host_prog,
                                int32_t n_stage, const uint8_t* point_mask, void* stream);

/* Companion table of a per-level program, computed on the HOST (no device access), in two parts.
 * (1) Per 16-byte vector: out[s*C + c] is the operator shared by the levels c*V .. c*V+V-1 of stage s (V = 16 bytes /
 *     sizeof(dtype), C = ceil(n_lev / V); padding levels join any operator), with op = ATX_OP_MIXED (and use_mask = whether any
 *     of them uses the mask) where they differ once the parameters are rounded to dtype.
 * (2) From the next 16-byte boundary after those n_stage*C entries: the operators of EVERY level in the stack's arithmetic type,
 *     parameters and codes apart — p0[n_stage][C*V], p1[n_stage][C*V] (float or double), code[n_stage][C*V] (one byte:
 *     op | use_mask << 7; the padding of the last vector repeats the last level) — so that a lane reads the parameters of its
 *     vector's levels with two 16-byte loads: programs with a different scale per level (packed surface stacks, normalisation
 *     per level) then cost the fused regrid epilogue nothing extra (O1280 -> 0.25 deg, 137 levels: 0.44 ms with or without).
 * Returns the size of the whole table in atx_level_op entries (out == NULL: only that — always size `out` by this query);
 * out_entries is the capacity of `out` in entries: ATX_EWORKSPACE, and nothing written, when it is smaller than the table.
 * Negative on error.  Uploaded to a 16-byte aligned device buffer and passed as `vec_prog` (of the stack's dtype) it lets
 * atx_regrid_ell fuse multiply-add programs on its fastest kernel and atx_pointwise_stack run without any per-workgroup set-up;
 * vec_prog == NULL is always valid (the kernels then derive what they need themselves). */
#define ATX_OP_MIXED (-1)
ATX_API int64_t atx_vector_program(const atx_level_op* prog, int32_t n_stage, int64_t n_lev, int dtype, atx_level_op* out, int64_t out_entries);

/* ---- multi-input per-point transforms ------------------------------------------ */
/* Operators of the reference's MatchingFieldsFilter family (R: filters/fields/matching.py:90-311):
 * every input / output is a stack of the same shape, pitch and layout; level l of the
 * outputs is computed from level l of the inputs (the fields of one matching group). */
typedef enum {
    ATX_COMB_SNOW_DEPTH_M = 0, /* (sd, rsn) -> 1000.0*sd/rsn            R: filters/fields/snow_depth_m.py:42      */
    ATX_COMB_SNOW_COVER = 1,   /* (sd, rsn) -> clip(tanh(4000*(1000*sd/rsn)/clip(rsn,100,400)),0,1), >0.99 -> 1
                                                                        R: filters/fields/snow_cover.py:34-39     */
    ATX_COMB_COS_SIN = 2,      /* (x) -> (cos x, sin x); flag ATX_COMB_DEGREES: x = deg2rad(x) first
                                  R: filters/fields/cos_sin_from_rad.py:78-79, cos_sin_mean_wave_direction.py:72-76 */
    ATX_COMB_ATAN2 = 3,        /* (cos, sin) -> atan2(sin, cos); flag ATX_COMB_DEGREES: rad2deg, then wrap to [0, 360)
                                  R: cos_sin_from_rad.py:100, cos_sin_mean_wave_direction.py:97-99                 */
    ATX_COMB_W_TO_WZ = 4,      /* (w, t, q) -> (-1/(rho*g + 1e-8))*w, rho = (100*level)/(287*t*(1+0.61*q) + 1e-8)
                                  level = level_param[l]              R: filters/fields/w_to_wz.py:97-99          */
    ATX_COMB_WZ_TO_W = 5,      /* (wz, t, q) -> -1.0*rho*g*wz          R: w_to_wz.py:124-126                       */
    ATX_COMB_SUM = 6,          /* (c0, c1, ...) -> ((c0 + c1) + ...) in input order   R: filters/fields/sum.py:109-116 */
    ATX_COMB_SUB = 7,          /* (a, b) -> a - b                      R: filters/fields/accum_to_interval.py:98   */
    ATX_COMB_XY_TO_POLAR = 8,  /* (u, v) -> (hypot(u, v), mod(270 - atan2(v, u)*180/pi, 360)): speed and the direction the wind blows FROM,
                                  the "meteo" convention of earthkit.meteo.wind.array.xy_to_polar      R: filters/fields/uv_to_ddff.py:93-97   */
    ATX_COMB_POLAR_TO_XY = 9,  /* (speed, dir) -> (speed*cos(a), speed*sin(a)), a = (270 - dir)*pi/180   R: uv_to_ddff.py:121-125         */
    /* 0.4.1: the reference's remaining numpy-only per-point filters */
    ATX_COMB_OPERA_CLIP = 10,  /* (tp, qi) -> (c(tp, max)/1000, c(qi, 1)), c(v, m): v<0 -> 0, then v>=m -> m (NaN and -0.0 kept);
                                  max = level_param[l]    R: filters/fields/rodeo_opera_clipping.py:92-98, rodeo_opera_preprocessing.py:34-37 */
    ATX_COMB_OPERA_PREPROCESS = 11, /* (tp, qi, dm) -> (c(tp', max), c(qi', 1)); tp' = NaN where dm is 1 or 3, 0 where dm is 2; qi' = 0 where
                                  dm is 2; max = level_param[l]                R: rodeo_opera_preprocessing.py:83-87, :190-200        */
    ATX_COMB_ORAS6 = 12,       /* (x, siconc) -> x cleaned where siconc <= 1e-5; inputs[1] is ONE contiguous field [n_pts] shared by every
                                  level; level_param[l] = what level l is, an ATX_ORAS6_* code    R: filters/fields/oras6_clipping.py:189-215 */
    ATX_COMB_LOOKUP = 13,      /* (class) -> table[class]; level_param = double[1 + n]: n, then the value of class 0 .. n-1; a class that is
                                  not one of 0 .. n-1 (the reference's KeyError) gives NaN        R: filters/fields/land_parameters.py:71 */
    /* humidity conversions: the arithmetic is earthkit-meteo's (thermo.array; IFS saturation formulas), restated from its published form */
    ATX_COMB_R_TO_D = 14,      /* (r %, t) -> dewpoint: r == 0 -> 1e-4 first; e = r*es_water(t)/100; T(e) = (32.19 ln(e/611.21) - 17.502*273.16) /
                                  (ln(e/611.21) - 17.502)                               R: filters/fields/dewpoint.py:59-65               */
    ATX_COMB_D_TO_R = 15,      /* (td, t) -> 100*es_water(td)/es_water(t)                R: dewpoint.py:67-72                              */
    ATX_COMB_Q_TO_R = 16,      /* (q, t) or (q, t, p) -> 100*e/es_mixed(t), e = p q/(eps + (1-eps) q), eps = 287.0597/461.5250; without a
                                  pressure operand p = 100*level_param[l] (levelist, hPa)   R: filters/fields/q_to_r.py:70-75, q_height.py:117-121 */
    ATX_COMB_R_TO_Q = 17,      /* (r, t) or (r, t, p) -> eps e/(p - (1-eps) e), e = r*es_mixed(t)/100; NaN where p - e < 1e-4
                                                                                         R: q_to_r.py:77-83, q_height.py:138-142           */
    ATX_COMB_Q_TO_D = 18,      /* (q, p) -> dewpoint: q == 0 -> 1e-8 first (on the operand, not in the input); e = p q/(eps + (1-eps) q), then
                                  the inverse of es_water as ATX_COMB_R_TO_D               R: q_height.py:466-475 (EPS_SPECIFIC, :25)        */
    ATX_COMB_D_TO_Q = 19,      /* (td, p) -> eps e/(p - (1-eps) e), e = es_water(td); NaN where p - e < 1e-4   R: q_height.py:511-514      */
    ATX_COMB_COUNT_ = 20
} atx_comb;
#define ATX_COMB_DEGREES 1
#define ATX_COMB_MAX_INPUTS 8
/* what a level of an ATX_COMB_ORAS6 stack holds (R: oras6_clipping.py:196-215) */
#define ATX_ORAS6_KEEP 0        /* passed on as it is (siconc itself)                                    */
#define ATX_ORAS6_ZERO 1        /* 0 where there is no ice (velocities, salinity, pressure, volumes, albedo) */
#define ATX_ORAS6_TEMPERATURE 2 /* 273.15 where there is no ice (sitemptop, sntemp, vasit)                   */
#define ATX_ORAS6_CELSIUS 3     /* a snow temperature archived in Celsius: + 273.15 first, then as above (:190-191) */
#define ATX_ORAS6_HEAT 4        /* 0 where there is no ice, then 0 wherever the value is >= -1e-5 (sihc, snhc) */
#define ATX_ORAS6_SURFACE 5     /* tos: raised to 271.15 - 1e-5 where it is at or below it; the ice mask is not used */
/* inputs / outputs: HOST arrays of n_in / n_out DEVICE pointers (n_in <= ATX_COMB_MAX_INPUTS, n_out <= 2).
 * level_param: device double[n_lev] or NULL (required by the W/WZ operators and by operators 10 to 13, which say above what they
 * read from it, and by operators 16 / 17 when they get no pressure operand).
 * All stacks share n_pts, n_lev, pitch and layout; the padding of the outputs (elements between a row's length and the pitch) is
 * written with zeros. */
ATX_API int atx_combine_stack(int op, const void* const* inputs, int32_t n_in, void* const* outputs, int32_t n_out,
                              int64_t n_pts, int64_t n_lev, int64_t pitch, int dtype, int layout,
                              const double* level_param, int32_t flags, void* stream);

/* ---- vertical reductions ------------------------------------------------------ */
/* out[p] = the pressure (Pa) at `height` metres above the ground of point p, from the model-level temperature `t` and specific humidity
 * `q` (two stacks of n_lev levels sharing pitch and layout, level 0 the TOP level: the reference orders them level="ascending"
 * first), the surface pressure `sp` (device [n_pts], dtype) and the hybrid half-level coefficients A, B (DEVICE double[n_lev + 1]).
 * earthkit-meteo's vertical.pressure_at_height_levels with alpha_top="ifs" and the moist gas constant Rd (1 - q) + Rv q, restated:
 * the statement is in atx_vertical.hip.  Evaluated in float64 for both dtypes; `out` is device [n_pts], dtype.  Every column is
 * walked to the top (the level count of the statement spans the whole column).
 *   R: filters/fields/q_height.py:203-213, :416-426 -> vertical.pressure_at_height_levels */
ATX_API int atx_pressure_at_height_stack(const void* t, const void* q, const void* sp, const double* A, const double* B,
                                         int64_t n_pts, int64_t n_lev, int64_t pitch, int dtype, int layout, double height,
                                         void* out, void* stream);

/* ---- vector frames ----------------------------------------------------------- */
/* (x_out[p, l], y_out[p, l]) = the vector (x[p, l], y[p, l]) mapped by the 2x2 frame of point p, shared by every level: the wind
 * components of one projection's axes in another's (rotate_winds / unrotate_winds).  The host builds the frame table in float64
 * (anemoi-transform_amd/projections.py) and casts it to `dtype`; it is DEVICE [n_pts, F], row-major, 16-byte aligned.
 * The statement, evaluated in `dtype` without contraction (numpy restates it bit for bit: projections.apply_frame):
 *   ATX_FRAME_ROTATION  F = 2, (c, s):               (c*u - s*v, s*u + c*v)
 *   ATX_FRAME_GENERAL   F = 4, (m00, m01, m10, m11): mx = m00*u + m01*v, my = m10*u + m11*v,
 *                                                    k = sqrt(u*u + v*v) / sqrt(mx*mx + my*my), result (mx*k, my*k)
 *   u == v == 0 (either sign): the result is the input, signed zeros kept.  NaN propagates.  (GENERAL: a vector so small that
 *   u*u + v*v underflows to zero, |w| below ~1e-19 in float32, gives NaN, as the statement does in numpy.)
 * x, y, x_out, y_out share n_pts, n_lev, pitch and layout; x_out == x and y_out == y (in place) are allowed, x_out == y_out is
 * not.  The padding of the outputs (elements between a row's length and the pitch) is written with zeros.
 *   R: filters/fields/rotate_winds.py:61-118 -> earthkit.geo.rotate.rotate_vector */
typedef enum { ATX_FRAME_ROTATION = 0, ATX_FRAME_GENERAL = 1 } atx_frame;
ATX_API int atx_rotate_vectors_stack(const void* x, const void* y, void* x_out, void* y_out, const void* frame, int frame_kind,
                                     int64_t n_pts, int64_t n_lev, int64_t pitch, int dtype, int layout, void* stream);

/* ---- observation gridding ---------------------------------------------------- */
/* winner[t * n_cells + c] = the row of the observation table that target time t shows in grid cell c, -1 when none: a keyed
 * arg-min over scattered rows (irregular_to_grid).  Row r takes part in target t when
 *   date_ns[r] and target_ns[t] are not NaT (INT64_MIN), not every one of its n_cols values is NaN, 0 <= cell[r] < n_cells, and
 *   target_ns[t] + before_ns  <  date_ns[r]  <  target_ns[t] + after_ns     (<= at an end whose closed_* flag is non-zero);
 * its score is  s = (double)|date_ns[r] - target_ns[t]| / (double)freq_ns,  and for w > 0
 *   (1.0 - w) * s + w * ((double)nan_count / (double)n_cols)                (two products, one sum, no contraction);
 * the winner of a cell is the row of smallest score, the SMALLEST ROW INDEX among equal scores (pandas idxmin on a table in
 * row order).  A row may win in several targets.  Cells outside [0, n_cells) are skipped, never used as an address.
 * Two order-independent atomic minima (the score's bit pattern, then the row index): the result is deterministic.
 *   date_ns, cell   device int64 [n_obs]           values      device double, n_cols columns of n_obs, column j at values + j * val_pitch
 *   target_ns       device int64 [n_time]          best        device scratch, n_time * n_cells uint64 (initialised by the call)
 *   winner          device int32 [n_time * n_cells] (initialised by the call: n_obs == 0 leaves it all -1)
 * n_obs >= 2^31, freq_ns <= 0 or w outside [0, 1]: ATX_EINVAL.
 *   R: filters/tabular/irregular_to_grid.py:139-159 -> select_window :209-254, get_nearest_obs :256-317 */
ATX_API int atx_obs_best_per_cell(const int64_t* date_ns, const int64_t* cell, const double* values, int64_t n_obs, int32_t n_cols,
                                  int64_t val_pitch, const int64_t* target_ns, int32_t n_time, int64_t n_cells, int64_t before_ns,
                                  int64_t after_ns, int closed_before, int closed_after, int64_t freq_ns, double w,
                                  uint64_t* best, int32_t* winner, void* stream);

/* Level t * n_cols + j of the float64 stack `out` (n_time * n_cols levels over n_cells points, either layout) at point c =
 * values[j * val_pitch + winner[t * n_cells + c]], NaN where the winner is not a row of the table (-1).  The padding of `out` is
 * written with zeros.
 *   R: filters/tabular/irregular_to_grid.py:135 (grids of NaN), :190-207 (_fill_grids), :163-188 (fields time-major, then column) */
ATX_API int atx_obs_fill_stack(const int32_t* winner, const double* values, int64_t n_obs, int32_t n_cols, int64_t val_pitch,
                               int32_t n_time, int64_t n_cells, double* out, int64_t pitch, int layout, void* stream);

/* ---- observation thinning (superob) ------------------------------------------ */
/* mean[c * out_pitch + g], count[c * out_pitch + g] = pandas' group mean of column c over the rows of group g, and the number of
 * rows that took part.  The rows of group g are order[offsets[g] .. offsets[g + 1]), ascending within the group (a STABLE sort
 * of the rows by group): the sum is taken in that order, one Kahan chain per group and column,
 *   y = v - comp;  t = sum + y;  comp = (t - sum) - y;  if comp is NaN, comp = 0;  sum = t;        mean = sum / count
 * with NaN values skipped (pandas/_libs/groupby.pyx group_mean; no contraction).  A group and column without a non-NaN row
 * gives NaN and count 0.  The chain is never split or reordered, so the result equals `df.groupby(keys)[cols].mean()` bit for
 * bit and does not depend on the launch shape; no atomics.  Integer and datetime columns go in converted to double (NaT as NaN).
 *   values   device double, n_cols columns of n_obs, column c at values + c * val_pitch
 *   order    device int32 [n_sel]: row indices (n_sel <= n_obs: dropped rows are simply absent); entries outside [0, n_obs) are
 *            skipped like NaN, never used as an address
 *   offsets  device int64 [n_groups + 1], 0 = offsets[0] <= ... <= offsets[n_groups] = n_sel (the caller's contract; a group whose
 *            bounds leave [0, n_sel] or run backwards gives NaN / 0)
 *   mean     device double, count device int64: n_cols rows of n_groups, out_pitch elements apart
 * n_obs >= 2^31 or n_cols outside 1 .. 65535: ATX_EINVAL.  val_pitch < n_obs, out_pitch < n_groups, n_sel > n_obs or
 * n_groups > n_sel: ATX_ESHAPE.
 *   R: filters/tabular/superob.py:86 `df.groupby(groupby_cols, observed=True, sort=False)[columns_to_average].mean()` */
ATX_API int atx_obs_group_mean(const double* values, int64_t n_obs, int32_t n_cols, int64_t val_pitch, const int32_t* order, int64_t n_sel,
                               const int64_t* offsets, int64_t n_groups, double* mean, int64_t* count, int64_t out_pitch, void* stream);

/* nearest[g] = the row of group g with the smallest distance, the FIRST such row in the group's order among equals (pandas
 * idxmin on a table in row order); a NaN distance is chosen only when the group has nothing else (then: its first row); -1 for
 * a group with bad bounds.  order / offsets as for atx_obs_group_mean.
 *   R: filters/tabular/superob.py:88 `df.groupby(groupby_cols, observed=True, sort=False)["distance"].idxmin()` */
ATX_API int atx_obs_group_argmin(const double* distance, int64_t n_obs, const int32_t* order, int64_t n_sel, const int64_t* offsets,
                                 int64_t n_groups, int32_t* nearest, void* stream);

/* ---- per-row observation operators (forcings, view angles, brightness temperature) ---- */
/* float64, one lane per row, n == 0 is a no-op.  Every statement is evaluated in the operation order of the reference's source, with
 * IEEE division and no contraction: the calendar, the arguments of the trigonometric functions and numpy's `%` have numpy's bits;
 * cos / sin are the library's own routine for |x| < 1e5 (< 1 ulp), the device library's otherwise, asin / acos / atan / log1p the
 * device library's.  Outputs are rows of ONE block: requested output k (in the order of its bit) at out + k * pitch.
 *
 * atx_obs_forcings: the nine columns of add_forcings, chosen by `mask`:
 *   bit 0 cos_julian_day   1 sin_julian_day   2 cos_sza   3 sin_local_time   4 cos_local_time
 *   bit 5 cos_latitude     6 sin_latitude     7 cos_longitude   8 sin_longitude
 * julian_day = whole days since 1 January of the date's year + whole seconds of the day / 86400.0 (integer calendar; sub-second parts
 * dropped, as Timedelta.seconds drops them; dates before 1970 are negative nanoseconds); hours = that day fraction * 24.  NaT
 * (INT64_MIN) gives NaN in every date-dependent column.  cos_sza is clipped at 0.  Columns a mask does not need may be NULL.
 *   date_ns    device int64 [n], nanoseconds since the epoch     latitude, longitude   device double [n], degrees
 *   out        device double, popcount(mask) rows of n, pitch elements apart
 * mask == 0 or bits beyond the nine, n < 0: ATX_EINVAL.  pitch < n: ATX_ESHAPE.
 *   R: filters/tabular/add_forcings.py:51-61 (names), :86-127 (angles), support/compute_forcings.py:14-87 (cos_sza) */
ATX_API int atx_obs_forcings(const int64_t* date_ns, const double* latitude, const double* longitude, int64_t n, uint32_t mask, double* out,
                             int64_t pitch, void* stream);

/* Viewing azimuth (flags bit 0) and zenith (bit 1) of a satellite at (sat_latitude, sat_longitude), per row, degrees; azimuth first
 * when both are asked for.  Azimuth: exactly 0.0 unless BOTH |latitude - sat_latitude| and |longitude - sat_longitude| exceed 0.00001
 * (a NaN fails the comparison); then the law of sines / cosines with minimum(1, sqrt(za)), the two clips to [-1, 1], the sign switch
 * on azmsin > 0, the two wraps by 2 pi, degrees and numpy's mod 360.  Zenith: a geostationary orbit, satalt from the source's literals.
 * flags outside 1 .. 3, n < 0: ATX_EINVAL.  pitch < n: ATX_ESHAPE.
 *   R: filters/tabular/support/sat_view_angles.py:52-97 (calc_azimuth), :17-49 (calc_zenith); add_azimuth.py:57-60, add_msg_angles.py:74-80 */
ATX_API int atx_obs_view_angles(const double* latitude, const double* longitude, const double* sat_latitude, const double* sat_longitude,
                                int64_t n, uint32_t flags, double* out, int64_t pitch, void* stream);

/* out[c * out_pitch + i] = b[c] / log1p(a[c] / max(radiance[c * in_pitch + i] * 1e-2, 1e-300)): CrIS radiances in mW/(m^2 sr cm^-1) to
 * brightness temperatures in K, one row per channel; a = C1 nu^3 and b = C2 nu come from the host (a NaN wavenumber gives NaN, and
 * so does a NaN radiance; a zero, negative or tiny radiance is floored at 1e-300).  out may be radiance (in place).
 * n_ch outside 1 .. 65535, n < 0: ATX_EINVAL.  a pitch below n: ATX_ESHAPE.
 *   R: filters/tabular/radiance_to_brightness_temperature.py:96-113 */
ATX_API int atx_obs_planck_bt(const double* radiance, int64_t n, int32_t n_ch, int64_t in_pitch, const double* a, const double* b, double* out,
                              int64_t out_pitch, void* stream);

/* pix[i] = the HEALPix pixel of (longitude[i], latitude[i]) degrees at resolution nside, in the RING or the NESTED ordering: healpy's
 * ang2pix(nside, lon, lat, nest, lonlat=True), that is lonlat2thetaphi (theta = pi/2 - radians(lat), phi = radians(lon)) followed by
 * healpix_cxx's loc2pix, restated in float64 in the operation order of the source (Gorski et al. 2005, ApJ 622, 759).  Away from pixel
 * edges the index is the exact geometry's; on an edge the last bit of cos / sin of theta decides between the two neighbours.
 * A row without a pixel — latitude NaN or with theta outside [0, pi], longitude NaN or infinite — gets pix[i] = -1, and *n_bad
 * (device, set by this call whenever n > 0) counts such rows.
 *   longitude, latitude  device double [n], degrees
 *   nside                1 .. 2^29; ATX_HEALPIX_NEST needs a power of two, ATX_HEALPIX_RING takes any
 *   pix                  device int64 [n]
 * n < 0, nside out of range or not a power of two under NEST, a scheme other than the two, a null pointer with n > 0: ATX_EINVAL.
 *   R: filters/tabular/add_healpix.py:43-51 (NEST); filters/tabular/support/superob.py:28-40 (the RING order of "h<nside>" grids) */
typedef enum { ATX_HEALPIX_RING = 0, ATX_HEALPIX_NEST = 1 } atx_healpix_scheme;
ATX_API int atx_healpix_ang2pix(const double* longitude, const double* latitude, int64_t n, int64_t nside, int scheme /* atx_healpix_scheme */,
                                int64_t* pix, int64_t* n_bad, void* stream);

/* out[r] = altitude[r], bit for bit, unless altitude[r] is NaN or the sentinel 9999.0; then out[r] = heights[i, j] widened to double,
 * with i (j) the entry of the orography's latitude (longitude) axis nearest to latitude[r] (longitude[r]): the arg-min of the float64
 * square (a - q) * (a - q), which is what a one-dimensional cKDTree query returns.  No wrap-around in longitude; a query beyond an
 * axis end takes the end.  Both axes come SORTED ASCENDING with the permutation back to file order (axis[p] is entry perm[p] of the
 * file), heights in file order: heights[i * heights_pitch + j], 64-bit indices.
 * Which of two equally near entries cKDTree returns is an artefact of its build and is not decided here: where the square of either
 * sorted neighbour of the winner equals the winner's, flags[r] gets ATX_FILL_TIE_LATITUDE / ATX_FILL_TIE_LONGITUDE and out[r] holds the
 * value at the kernel's own candidate; the caller answers that axis again.  Without the bit the winner's square is strictly the axis'
 * smallest.  A row to fill whose latitude or longitude is NaN or infinite gets NaN and no flag (cKDTree refuses such a query).
 * counters (device int64 [3], zeroed and set by this call, n == 0 included): rows given a value from heights, rows among them with a
 * flag, rows to fill with a coordinate that is not finite.  Kept rows may hold anything in latitude / longitude.
 *   latitude, longitude, altitude   device double [n]
 *   lat_axis, lon_axis              device double [n_lat], [n_lon], strictly ascending and finite (the caller checks)
 *   lat_perm, lon_perm              device int32 [n_lat], [n_lon], permutations
 *   heights                         device float / double (dtype), n_lat rows of n_lon, heights_pitch elements apart
 *   out  device double [n]          flags  device uint8 [n], written for every row
 * n < 0, an axis length outside 1 .. 2^31 - 1, a dtype other than the two, a null pointer: ATX_EINVAL.  heights_pitch < n_lon: ATX_ESHAPE.
 *   R: filters/tabular/fill_heights.py:68-91 (the rows), filters/tabular/support/utils.py:24-55 (get_heights) */
enum { ATX_FILL_TIE_LATITUDE = 1, ATX_FILL_TIE_LONGITUDE = 2 };
ATX_API int atx_obs_fill_heights(const double* latitude, const double* longitude, const double* altitude, int64_t n, const double* lat_axis,
                                 const int32_t* lat_perm, int64_t n_lat, const double* lon_axis, const int32_t* lon_perm, int64_t n_lon,
                                 const void* heights, int64_t heights_pitch, int dtype /* atx_dtype */, double* out, uint8_t* flags,
                                 int64_t* counters, void* stream);

/* A program of up to ATX_MAX_COLUMN_OPS single-input functions over float64 columns of n rows, in ONE pass: for t = 0 .. n_ops - 1,
 *   x = src[t] < 0 ? in[t][r] : (the result of operation src[t] for row r);   y = f_op[t](x);   if (out[t]) out[t][r] = y;
 * which is what the reference's loop of numpy ufuncs over the columns of a DataFrame computes when a later transformation reads an
 * earlier one's target.  op[t] is an ATX_COLOP_* code:
 *   LOG       log(x)                        the library's own routine, <= 1 ulp
 *   LOG1P     log1p(x)                      the device library's, 1 ulp; x itself for |x| < 2^-54, correctly rounded (the library's log1p(-0.0) is +0.0)
 *   SAFE_LOG  log(x + 1e-10)                the sum rounded once in float64, as numpy's
 *   SQRT      sqrt(x)                       correctly rounded: numpy's bits
 *   EXP       exp(x)                        the library's own routine, <= 1 ulp
 *   ABS       fabs(x)                       the sign bit cleared: -0.0 -> +0.0, a NaN keeps its payload
 *   SIN, COS  sin(x), cos(x)                the library's own routine for |x| < 1e5 (< 1 ulp), the device library's beyond (2 ulps)
 *   SIN_DEG, COS_DEG  sin / cos(x * (pi / 180))   np.deg2rad's product, one rounding, then as SIN / COS
 * Specials are the functions' own: log(0) = -inf, log(-1) = NaN, log1p(-1) = -inf, sqrt(-0.0) = -0.0, exp overflows to inf,
 * sin(+-inf) = NaN.  No contraction anywhere.
 *   op, src   HOST int32 [n_ops]
 *   in, out   HOST arrays of n_ops DEVICE pointers to double [n]; they are copied into the kernel's arguments, so they may be freed on
 *             return.  in[t] is read only where src[t] < 0 (anything else there is ignored).  out[t] may be NULL: the result is an
 *             intermediate, taken by a later operation through src or replaced by a later operation with the same target.  out[t] may
 *             be any in[.] (in place): a lane loads a column before it stores to it, in program order.
 * The caller guarantees that no operation reads from memory a column that an EARLIER operation of the same call writes: that
 * dependency goes through src.  A column that a LATER operation writes may be read.
 * n_ops outside 1 .. ATX_MAX_COLUMN_OPS, an unknown code, src[t] >= t, in[t] == NULL where src[t] < 0 (n > 0), a null program array,
 * n < 0: ATX_EINVAL, nothing launched.  n == 0: validated, nothing launched.
 *   R: filters/tabular/apply_column_transformations.py:18-42 (the ten functions), :55-61 (apply), :132-138 (in order, chained)
 *
 * A SECOND FAMILY of codes, ATX_COLOP_SCALAR (16) and above, carries the tabular QC filters (R: filters/tabular/mask.py,
 * mask_outside_range.py, mask_infs.py, mask_dewpoint_temperature.py, exclude_dates.py, remove_extreme_values.py, clip.py, impute_nans.py,
 * drop_nans.py): compares, selects and one fabs per row, all exact.  A program is EITHER all codes 0 .. 9 OR all codes >= 16 (a mixed one
 * is ATX_EINVAL); codes 10 .. 15 and above 32 are unknown.  The slot fields mean what they mean above; x is in[t][r] or the result of
 * operation src[t].  New: a binary operation takes a second operand y = the result of operation t - 1 (whatever that is), so a binary
 * operation at t = 0 is ATX_EINVAL.  Conditions are the doubles 0.0 / 1.0.
 *   SCALAR      in[t][0] for every row           in[t] is a DEVICE double read at element 0 only; src[t] must be < 0 (else ATX_EINVAL)
 *   COPY        x                                the bits kept, NaN payloads included
 *   IS_NAN      x != x ? 1 : 0
 *   NOT         x == 0 ? 1 : 0
 *   CMP_GT, CMP_LT, CMP_EQ, CMP_NE, CMP_GE, CMP_LE   (x cmp y) ? 1 : 0     ATX_COLOP_CMP_GT + atx_cmp; IEEE's and numpy's compares:
 *                                                false whenever x or y is a NaN, except NE, which is then true
 *   ABS_GT      fabs(x) > y ? 1 : 0
 *   AND, OR     (x != 0) and / or (y != 0) ? 1 : 0    a NaN is not 0
 *   NAN_WHERE   y != 0 ? the canonical quiet NaN 0x7ff8000000000000 : x      pandas' Series.mask(y)
 *   CLIP_LOW    x < y ? y : x                    selects, not fmax / fmin: a NaN x stays, and so does -0.0 against a bound of 0.0
 *   CLIP_HIGH   x > y ? y : x
 *   FILL_NAN    x != x ? y : x                   pandas' Series.fillna(y)
 * Every select hands on the bits of the operand it picks. */
#define ATX_MAX_COLUMN_OPS 16
enum {
    ATX_COLOP_LOG = 0,
    ATX_COLOP_LOG1P = 1,
    ATX_COLOP_SAFE_LOG = 2,
    ATX_COLOP_SQRT = 3,
    ATX_COLOP_EXP = 4,
    ATX_COLOP_ABS = 5,
    ATX_COLOP_SIN = 6,
    ATX_COLOP_SIN_DEG = 7,
    ATX_COLOP_COS = 8,
    ATX_COLOP_COS_DEG = 9,
    /* 10 .. 15: unknown */
    ATX_COLOP_SCALAR = 16,
    ATX_COLOP_COPY = 17,
    ATX_COLOP_IS_NAN = 18,
    ATX_COLOP_NOT = 19,
    ATX_COLOP_CMP_GT = 20, /* 20 + atx_cmp: GT, LT, EQ, NE, GE, LE */
    ATX_COLOP_CMP_LT = 21,
    ATX_COLOP_CMP_EQ = 22,
    ATX_COLOP_CMP_NE = 23,
    ATX_COLOP_CMP_GE = 24,
    ATX_COLOP_CMP_LE = 25,
    ATX_COLOP_ABS_GT = 26,
    ATX_COLOP_AND = 27,
    ATX_COLOP_OR = 28,
    ATX_COLOP_NAN_WHERE = 29,
    ATX_COLOP_CLIP_LOW = 30,
    ATX_COLOP_CLIP_HIGH = 31,
    ATX_COLOP_FILL_NAN = 32
};
ATX_API int atx_obs_column_ops(int32_t n_ops, const int32_t* op, const int32_t* src, const double* const* in, double* const* out, int64_t n,
                               void* stream);

/* ---- row expressions: filter_query and mask_values_custom ---- */

/* A POSTFIX program over float64 columns of n rows, evaluated per row on a stack of at most ATX_EXPR_MAX_STACK values in ONE pass.  The
 * program is flat: instruction t is code[t] (an atx_expr_op) with its operands arg0[t] and arg1[t]; an operand a code does not use is
 * ignored.  code, arg0, arg1, in, consts and out are HOST arrays, read during the call.
 *   PUSH_COL           push in[arg0][row]; in: n_inputs (at most ATX_EXPR_MAX_INPUTS) DEVICE columns of n doubles
 *   PUSH_CONST         push consts[arg0]; consts: n_consts (at most ATX_EXPR_MAX_CONSTS) HOST doubles, copied during the call
 *   ADD SUB MUL DIV    (x, y) -> x op y, y the top: IEEE float64, one rounding each, never contracted
 *   NEG ABS            the sign bit flipped / cleared           ROUND_F32      (double)(float)x: round to nearest even, subnormals kept
 *   CMP_GT .. CMP_LE   (x, y) -> (x cmp y) ? 1 : 0, ATX_EXPR_CMP_GT + atx_cmp; IEEE's compares: false against a NaN, except NE
 *   IN_SET             x -> 1 if x == consts[j] for a j in [arg0, arg0 + arg1), arg1 >= 1, else 0 (a NaN equals nothing; -0.0 == 0.0)
 *   AND OR             (x, y) -> 0 / 1, an operand is true when it is not 0        NOT   x -> (x == 0) ? 1 : 0
 *   DUP                push a copy of the value arg0 below the top (0: the top)    SWAP  exchange the top two
 *   NAN_WHERE          (x, c) -> the canonical quiet NaN 0x7ff8000000000000 where c is not 0, else the BITS of x
 * Results: stack slot r (counted from the bottom) of what the program leaves, r < n_results <= ATX_EXPR_MAX_RESULTS, is stored to the
 * device row out[r], which may be any input column (a lane loads its row before it stores it).  With keep != 0 one more slot, on top of
 * the results, is the row's keep condition:
 *   keep_words    device uint64 [ceil(n / 64)]: bit (row % 64) of word (row / 64) is set where the condition is not 0; the bits past
 *                 n of the last word are 0
 *   chunk_counts  device int64 [ceil(n / ATX_EXPR_CHUNK_ROWS)]: the rows kept in every chunk
 * Every word and every count is written by exactly one lane: no atomics, no order between workgroups.  With keep == 0 both are ignored.
 * ATX_EINVAL, nothing launched: n < 0; a null code, arg0 or arg1; n_instr outside 1 .. ATX_EXPR_MAX_INSTR; n_inputs, n_consts or
 * n_results negative or above its limit; neither a result nor keep; a null in, consts or out with a count above 0; an unknown code; a
 * column or constant index outside its table, an IN_SET slice outside consts or of fewer than 1 member; a stack that underflows or
 * grows beyond ATX_EXPR_MAX_STACK (the depth is simulated on the host); a final depth other than n_results (+ 1 with keep); a null
 * column, output or keep row with n > 0.  n == 0: validated, nothing launched, ATX_OK.
 *
 * atx_obs_keep_positions lists the kept rows: positions[j] (device int64 [n_positions]) = the j-th row, ascending, whose bit is set in
 * keep_words (over n rows); chunk_offsets is the EXCLUSIVE prefix sum of the chunk counts (device int64).  A row's place is its
 * chunk's offset plus the number of set bits below it in its chunk; a place outside [0, n_positions) is not written.  One lane per
 * row, plain stores, no workgroup waits for another.  n < 0 or n_positions < 0: ATX_EINVAL.  n == 0 or n_positions == 0: nothing
 * launched, ATX_OK.  Otherwise a null pointer: ATX_EINVAL.
 *   R: filters/tabular/filter_query.py:76-92 (obs_df.query(query)); filters/tabular/mask_values_custom.py:47-67
 *   (obs_df.eval(condition), Series.mask) */
#define ATX_EXPR_MAX_INPUTS 16
#define ATX_EXPR_MAX_INSTR 32
#define ATX_EXPR_MAX_CONSTS 64
#define ATX_EXPR_MAX_STACK 8
#define ATX_EXPR_MAX_RESULTS 4
#define ATX_EXPR_CHUNK_ROWS 256
typedef enum {
    ATX_EXPR_PUSH_COL = 0,
    ATX_EXPR_PUSH_CONST = 1,
    ATX_EXPR_ADD = 2,
    ATX_EXPR_SUB = 3,
    ATX_EXPR_MUL = 4,
    ATX_EXPR_DIV = 5,
    ATX_EXPR_NEG = 6,
    ATX_EXPR_ABS = 7,
    ATX_EXPR_ROUND_F32 = 8,
    ATX_EXPR_CMP_GT = 9, /* 9 + atx_cmp: GT, LT, EQ, NE, GE, LE */
    ATX_EXPR_CMP_LT = 10,
    ATX_EXPR_CMP_EQ = 11,
    ATX_EXPR_CMP_NE = 12,
    ATX_EXPR_CMP_GE = 13,
    ATX_EXPR_CMP_LE = 14,
    ATX_EXPR_IN_SET = 15,
    ATX_EXPR_AND = 16,
    ATX_EXPR_OR = 17,
    ATX_EXPR_NOT = 18,
    ATX_EXPR_DUP = 19,
    ATX_EXPR_SWAP = 20,
    ATX_EXPR_NAN_WHERE = 21
} atx_expr_op;
ATX_API int atx_obs_row_expr(int32_t n_instr, const int32_t* code, const int32_t* arg0, const int32_t* arg1, int32_t n_inputs,
                             const double* const* in, int32_t n_consts, const double* consts, int32_t n_results, double* const* out, int keep,
                             uint64_t* keep_words, int64_t* chunk_counts, int64_t n, void* stream);
ATX_API int atx_obs_keep_positions(const uint64_t* keep_words, const int64_t* chunk_offsets, int64_t n, int64_t* positions,
                                   int64_t n_positions, void* stream);

/* ---- row sets: pandas' order and equality as int64 keys, first occurrences, a gather of rows ---- */

/* key[i] = the int64 ORDER KEY of column[i], defined by two properties: key(a) < key(b) exactly when pandas' sort_values puts a before b,
 * and key(a) == key(b) exactly when pandas' drop_duplicates treats a and b as the same value.  That rule is not IEEE's: -0.0 and 0.0
 * are one key; every NaN, whatever its sign or payload, is one key and the LAST (INT64_MAX), and so is NaT; +-inf order as numbers
 * (+inf stays below the NaN key); integers compare as integers (2^53 and 2^53 + 1 differ).  dtype is an atx_key_dtype:
 *   F64, F32        the sign-magnitude to two's-complement map of the float64 bit pattern (float32 widened first, which is exact)
 *   I64 .. I8, U8   the value;   BOOL: 0 / 1 (any non-zero byte is true)
 *   DATETIME        int64 nanoseconds, NaT = INT64_MIN -> INT64_MAX (the one date that shares the key is INT64_MAX nanoseconds itself,
 *                   pandas' Timestamp.max, 2262-04-11T23:47:16.854775807)
 * Integer and compare work only: no rounding anywhere.  The same key serves the sort and the duplicate test.
 *   column  device, n elements of the dtype       key  device int64 [n]
 * n < 0, a dtype code outside the enum, a null pointer with n > 0: ATX_EINVAL.
 *   R: filters/tabular/sort_by.py:44-51 (df.sort_values(by=columns, kind="stable")); filters/tabular/drop_duplicates.py:49-61 */
#define ATX_MAX_ROWSET_COLUMNS 16
typedef enum {
    ATX_KEY_F64 = 0,
    ATX_KEY_F32 = 1,
    ATX_KEY_I64 = 2,
    ATX_KEY_I32 = 3,
    ATX_KEY_I16 = 4,
    ATX_KEY_I8 = 5,
    ATX_KEY_U8 = 6,
    ATX_KEY_BOOL = 7,
    ATX_KEY_DATETIME = 8
} atx_key_dtype;
ATX_API int atx_obs_order_key(const void* column, int64_t n, int dtype /* atx_key_dtype */, int64_t* key, void* stream);

/* keep[order[i]] = (i == 0) or there is a k < n_keys with keys[k][order[i]] != keys[k][order[i - 1]], for i < n.  With `order` the
 * STABLE sort of the rows by the key tuple, the rows marked are the first row of every set of rows equal in the keys, in table
 * order: pandas' df.drop_duplicates(subset), keep="first".  accumulate = 0 writes 0 or 1 to every keep[order[i]]; accumulate = 1
 * only ever SETS bytes (keep |= ...), for a tuple of more than ATX_MAX_ROWSET_COLUMNS keys taken 16 per launch.  An entry of
 * order outside [0, n) is not read through and marks nothing.
 *   keys    HOST array of n_keys DEVICE pointers to int64 [n] (copied into the kernel's arguments; may be freed on return)
 *   order   device int64 [n], a permutation of 0 .. n - 1        keep  device uint8 [n]
 * n < 0, n_keys outside 1 .. ATX_MAX_ROWSET_COLUMNS, accumulate other than 0 / 1, a null table, a null pointer with n > 0: ATX_EINVAL.
 *   R: filters/tabular/drop_duplicates.py:49-61 (obs_df.drop_duplicates(subset=subset)) */
ATX_API int atx_obs_mark_first(int32_t n_keys, const int64_t* const* keys, const int64_t* order, int64_t n, int accumulate, uint8_t* keep,
                               void* stream);

/* out[c][i] = in[c][rows[i]] for c < n_cols, i < n_out: the rows of a table of n_in rows at the positions `rows`, every column in one
 * pass — rows[i] is read once per row for all columns of the call.  width[c] is the element size of column c in bytes, 1, 2, 4 or 8,
 * mixed freely; elements are copied bit for bit.  A row index outside [0, n_in) is never read through: that output row is left
 * untouched in every column, and *n_bad (device, set by this call whenever n_out > 0) counts such rows.
 *   in, out   HOST arrays of n_cols DEVICE pointers (copied into the kernel's arguments); no output may overlap an input or rows
 *   width     HOST int32 [n_cols]        rows  device int64 [n_out]
 * n_out < 0, n_in < 0, n_cols outside 1 .. ATX_MAX_ROWSET_COLUMNS, a width other than the four, a null table or n_bad, a null column or
 * rows with rows to take: ATX_EINVAL, nothing launched.
 *   R: filters/tabular/sort_by.py:51 (the frame sort_values returns), filters/tabular/drop_duplicates.py:61 (the frame
 *   drop_duplicates returns): every column of the table at the chosen rows */
ATX_API int atx_obs_take_rows(int32_t n_cols, const void* const* in, void* const* out, const int32_t* width, const int64_t* rows,
                              int64_t n_out, int64_t n_in, int64_t* n_bad, void* stream);

/* ---- masks ------------------------------------------------------------------ */

/* mask[i] = (m[i*m_stride] CMP threshold) ? 1 : 0   for i < n.
 *   R: apply_mask.py:160-163  `OPERATORS[op](mask_values, threshold)` / `mask_values == mask_value`
 *   R: remove_nans.py:101     `~np.isnan(data)`  (ATX_CMP_NOTNAN)
 * m_stride in elements (1 for a flat field, the pitch for a level of an ATX_COLUMNS stack). */
ATX_API int atx_mask_build(const void* m, int64_t m_stride, uint8_t* mask, int64_t n, int cmp, double threshold,
                           int dtype, void* stream);

/* *count (device int64) = number of non-zero mask bytes.  R: numpy boolean indexing output size. */
ATX_API int atx_mask_count(const uint8_t* mask, int64_t n, int64_t* count, void* stream);

/* Stable compaction: index[0..count) = ascending positions i with mask[i] != 0;
 * *count (device int64) receives the total.  The index list turns
 * `data[bool_mask]` into atx_regrid_ell(k=1, w=NULL).
 *   R: remove_nans.py:110-116, regrid.py:420 (boolean mask)
 * workspace: device scratch of at least atx_mask_to_index_workspace(n) bytes. */
ATX_API size_t atx_mask_to_index_workspace(int64_t n);
ATX_API int atx_mask_to_index(const uint8_t* mask, int64_t n, int32_t* index, int64_t* count,
                              void* workspace, size_t workspace_bytes, void* stream);

/* ---- reductions (range / validity checks) ---------------------------------- */
typedef enum { ATX_RED_MIN = 0, ATX_RED_MAX = 1, ATX_RED_NANCOUNT = 2, ATX_RED_MINMAX = 3 } atx_red;
/* result: device double[1] (double[2] for ATX_RED_MINMAX: minimum, maximum — both from ONE pass over the data);
 * min/max ignore nothing (NaN propagates like np.min); NANCOUNT returns the count as a double.
 *   R: filters/fields/cos_sin_from_rad.py:73-76 `data.min()/max()`;
 *      tests/field_filters/test_apply_mask.py:106 `np.sum(np.isnan(result))`
 * workspace (optional, NULL = none): device scratch of atx_reduce_workspace() bytes, 8-byte aligned, usable by one call at a time
 * per stream (no initialisation needed).  With it the workgroups store partials and a second one-workgroup launch combines them: no
 * per-workgroup atomics on `result`, no initialisation launch, and `result` may be a pinned HOST cell the caller reads after
 * synchronising the stream (no copy back) — for EVERY shape: lengths that are not a multiple of the 16-byte vector, unaligned
 * bases (two scalar passes for MINMAX) and empty input (the identities: +inf, -inf, 0).  Without a workspace the workgroups
 * combine through atomics on `result`, which must then be DEVICE memory. */
ATX_API size_t atx_reduce_workspace(void);
ATX_API int atx_reduce(const void* x, int64_t n, int red, double* result, int dtype, void* workspace, size_t workspace_bytes, void* stream);
/* the same over the n_pts x n_lev elements of a (pitched) stack, padding excluded */
ATX_API int atx_reduce_stack(const void* x, int64_t n_pts, int64_t n_lev, int64_t pitch, int red, double* result,
                             int dtype, int layout, void* workspace, size_t workspace_bytes, void* stream);

/* ---- k-nearest-neighbour index build ---------------------------------------- */
/* Exact k-NN on the unit sphere by chord distance — device counterpart of
 *   R: spatial.py:587-635  cKDTree(source_xyz).query(target_xyz, k [, distance_upper_bound])
 * xyz arrays are float64 [n, 3] computed on the host as R: spatial.py:132-167 does.
 * atx_knn_build sorts the sources along a Morton curve and builds an implicit box tree in
 * `workspace` (atx_knn_workspace_bytes(n_src) bytes, 256-byte aligned, owned by the caller,
 * reusable for any number of queries).  atx_knn_query writes, per target, the k nearest
 * source indices (int32, ascending distance, ties by lower index, n_src if fewer than k
 * exist) and their SQUARED distances, bit-identical to scipy's float64 arithmetic; k <= 17
 * (16 neighbours plus one to look ahead: a caller that needs cKDTree's own order among
 * EXACTLY equidistant candidates queries k+1, finds the rows with equal adjacent distances and
 * re-resolves those with cKDTree — what the host mirror's nearest_grid_points_device does). */
ATX_API size_t atx_knn_workspace_bytes(int64_t n_src);
ATX_API int atx_knn_build(const double* src_xyz, int64_t n_src, void* workspace, size_t workspace_bytes, void* stream);
ATX_API int atx_knn_query(const void* workspace, int64_t n_src, const double* tgt_xyz, int64_t n_tgt, int32_t k,
                          int32_t* idx_out, double* d2_out, void* stream);

/* ---- mask builders ------------------------------------------------------------- */
/* inside[i] = 1 if the ray from the Earth's centre through global point i hits any of the `k`
 * triangles (nb[i][j], nb[i][(j+1)%k], nb[i][(j+2)%k]) of its k nearest limited-area points
 * (Moeller-Trumbore, epsilon 1e-7) — the per-point loop of
 *   R: spatial.py:404-424 (cutout_mask) over R: spatial.py:186-233 (Triangle3D.intersect)
 * evaluated for all points at once.  global_xyz [n,3] and lam_xyz [n_lam,3] float64 unit-sphere
 * coordinates, neighbours int32 [n,k] (from atx_knn_query; k <= 17), inside uint8 [n].  A triangle with a vertex
 * index outside [0, n_lam) is skipped, never dereferenced. */
ATX_API int atx_cutout_inside(const double* global_xyz, int64_t n, const double* lam_xyz, int64_t n_lam,
                              const int32_t* neighbours, int32_t k, uint8_t* inside, void* stream);

/* ---- multi-GPU: the source exchange of a target-sharded regrid ------------------------ */
/* One process per GPU; RCCL (over xGMI on an MI355X node) is bound at first use (dlopen), so the library loads without
 * it.  The regrid path itself needs no collective: rows of the operator are independent, every rank computes a
 * contiguous slice of the target points (R: filters/fields/regrid.py:204-208 is a single-process loop — there is no
 * reference counterpart).  What has to travel is the SOURCE stack, once:
 *   atx_bcast          the whole pitched stack from its owner ("source broadcast once")
 *   atx_all_gather     every rank's stack onto every rank in one collective
 *   atx_exchange       or only the slab of source columns each peer's target slice references (ATX_COLUMNS: a
 *                      contiguous byte range), grouped send/recv — about 1/world of the bytes for lat-lon targets
 *   atx_gather_shards  optionally the target slices back onto every rank
 * All calls enqueue on `stream` of the CURRENT device and return; buffers are device memory owned by the caller.
 * A communicator belongs to the device that was current in atx_comm_init.  Errors: ATX_ECOMM + atx_last_error(). */
typedef struct atx_comm atx_comm;
#define ATX_COMM_ID_BYTES 128
/* RCCL's version code (e.g. 22205), or a negative status if RCCL cannot be loaded. */
ATX_API int atx_comm_version(void);
/* Rank 0 fills `id` (HOST, ATX_COMM_ID_BYTES) and hands it to every rank out of band (file, socket, MPI, a
 * torch.distributed store ...). */
ATX_API int atx_comm_unique_id(void* id);
/* Collective over all `world` ranks: join the job identified by `id` as `rank`, on the current HIP device. */
ATX_API int atx_comm_init(atx_comm** comm, int32_t world, int32_t rank, const void* id);
ATX_API int atx_comm_destroy(atx_comm* comm);
ATX_API int atx_comm_rank(const atx_comm* comm);
ATX_API int atx_comm_world(const atx_comm* comm);
/* buf[0..n_bytes) of rank `root` onto every rank, in place. */
ATX_API int atx_bcast(atx_comm* comm, void* buf, int64_t n_bytes, int32_t root, void* stream);
/* Every rank contributes send[0..bytes_per_rank); afterwards recv[p * bytes_per_rank ...) holds rank p's contribution on every rank
 * (recv: world * bytes_per_rank bytes; send may be the rank's own slot of recv).  The whole-stack exchange of a job in which every
 * rank owns one source stack, as ONE collective instead of `world` broadcasts. */
ATX_API int atx_all_gather(atx_comm* comm, const void* send, void* recv, int64_t bytes_per_rank, void* stream);
/* send_ptrs / send_bytes / recv_ptrs / recv_bytes: HOST arrays of `world` entries, one per peer; entry p of the send
 * side goes to rank p, entry p of the receive side is filled by rank p (byte counts must match pairwise across ranks;
 * zero skips the pair; the own entry is a device-to-device copy). */
ATX_API int atx_exchange(atx_comm* comm, const void* const* send_ptrs, const int64_t* send_bytes, void* const* recv_ptrs,
                         const int64_t* recv_bytes, void* stream);
/* byte_offsets: HOST array of world + 1 non-decreasing offsets into buf; rank p owns [byte_offsets[p], byte_offsets[p+1])
 * and has filled it; afterwards every rank holds all ranges (ATX_COLUMNS: a rank's target slice is such a range). */
ATX_API int atx_gather_shards(atx_comm* comm, void* buf, const int64_t* byte_offsets, void* stream);

/* ---- measurement aid ------------------------------------------------------------ */
/* dst[0..n_bytes) = src[0..n_bytes): a plain streaming copy, one 16-byte vector per lane, one workgroup per 4 KB, never
 * tuned again.  It exists so that profiling has a FIXED kernel with a known byte count in the library's access width:
 * tools/pmc_probe.py calibrates the FETCH_SIZE / WRITE_SIZE counters on it, tools/hbm_ceiling.py reports it as the
 * device's practical 1 read : 1 write rate.  n_bytes a multiple of 16, both pointers 16-byte aligned. */
ATX_API int atx_stream_copy(const void* src, void* dst, int64_t n_bytes, void* stream);

/* ---- layout --------------------------------------------------------------- */
/* dst[p, l] = src[p, l] between layouts / pitches (LDS-tiled transpose when the
 * layouts differ, strided copy when they agree).  No reference counterpart:
 * `field.to_numpy()` (R: fields.py:178-202) is the field-major view of a stack. */
ATX_API int atx_relayout(const void* src, void* dst, int64_t n_pts, int64_t n_lev,
                         int64_t src_pitch, int64_t dst_pitch, int src_layout, int dst_layout,
                         int dtype, void* stream);

/* dst level j = src level level_map[j] for j in [0, n_map); a negative entry leaves dst level j untouched.
 * Both stacks in `layout`; level_map is a HOST array (validated before launch, passed to the kernel by value).
 *   R: filter.py:188-196 / fields.py:35-48 — the reference re-lists fields freely (a FieldList is a Python
 *      list of independent arrays); on a stack, re-listing is this level gather. */
ATX_API int atx_select_levels(const void* src, void* dst, const int32_t* level_map, int32_t n_map, int64_t n_pts,
                              int64_t n_src_lev, int64_t src_pitch, int64_t dst_pitch, int dtype, int layout, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ATX_H */
