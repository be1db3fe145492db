// regrid_ell_typed<T> / regrid_csr_typed<T>, the two symbols atx_regrid.hip sees (atx_regrid_decl.hpp), over the two pieces of the
// gather: a column stack goes to atx_regrid_columns.inc, a field-major one to atx_regrid_fields.inc.  Included by atx_regrid_f32.hip
// and atx_regrid_f64.hip, which instantiate it for one element type each and compile in parallel.
#include <type_traits>

#include "atx_common.hpp"
#include "atx_regrid_decl.hpp"

#include "atx_regrid_columns.inc"
#include "atx_regrid_fields.inc"

namespace atx {

template <typename T>
int regrid_ell_typed(const EllBatch& batch, const int32_t* idx, const void* w_, int64_t n_tgt, int k,
                            int n_lev, int64_t sp, int64_t op, int layout, bool pad, const Epilogue& e, hipStream_t st) {
    const T* w = static_cast<const T*>(w_);
    if (layout == ATX_COLUMNS) return regrid_cols_ell<T>(batch, idx, w, n_tgt, k, n_lev, sp, op, pad, e, st);
    return regrid_fields_ell<T>(batch, idx, w, n_tgt, k, n_lev, sp, op, pad, e, st);
}

template <typename T>
int regrid_csr_typed(const void* src_, void* out_, const int32_t* indptr, const int32_t* indices,
                            const void* data_, int64_t n_tgt, int64_t nnz, int n_lev, int64_t sp, int64_t op,
                            int layout, const atx_level_op* prog, int n_stage, const uint8_t* m, const int32_t* rows, hipStream_t st) {
    const T* src = static_cast<const T*>(src_);
    T* out = static_cast<T*>(out_);
    const T* data = static_cast<const T*>(data_);
    if (layout == ATX_COLUMNS) return regrid_cols_csr<T>(src, out, indptr, indices, data, n_tgt, nnz, n_lev, sp, op, prog, n_stage, m, rows, st);
    return regrid_fields_csr<T>(src, out, indptr, indices, data, n_tgt, nnz, n_lev, sp, op, prog, n_stage, m, rows, st);
}

}  // namespace atx
