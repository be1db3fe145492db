// The tabular QC filters (mask_tabular, mask_outside_range, mask_infs, mask_dewpoint_temperature, exclude_dates, remove_extreme_values,
// clip_tabular, impute_nans_tabular, drop_nans_tabular): a program of compares, selects and row predicates over float64 columns, one
// launch.  It is the second family of atx_obs_column_ops' codes (ATX_COLOP_SCALAR .. ATX_COLOP_FILL_NAN, include/atx.h) and reaches the
// device through that entry point: same slots, same src / out rules, plus a second operand y for the binary operations — the result of
// the operation before it, one carried register.
//
// The reference (R: filters/tabular/mask.py, mask_outside_range.py, mask_infs.py, mask_dewpoint_temperature.py, exclude_dates.py,
// remove_extreme_values.py, clip.py, impute_nans.py, drop_nans.py: each one's forward) builds a boolean Series per condition and calls
// Series.mask / clip / fillna / dropna with it: a pass over the column per step.  Here a filter's whole statement for
// up to 16 slots is ONE pass: conditions are 0.0 / 1.0 in registers, and only what the caller asked for is stored.
//
// Arithmetic: compares, selects and one fabs — exact.  A select hands on the BITS of its operand (a NaN keeps its payload); the only
// value made here is NAN_WHERE's canonical quiet NaN, which is what Series.mask writes.  Compares are IEEE's and so numpy's: false
// against a NaN, except NE.  CLIP_LOW / CLIP_HIGH are written as selects, not fmax / fmin: a NaN x and -0.0 against 0.0 stay.
//
// Launch shape: the per-row kernels' (atx_obs_rows.hpp): kBlock lanes, row_grid, grid-stride, one lane per row.  The program is uniform
// over the launch: every branch on it is scalar.  Results stay in VGPRs: "the result of operation s" is the compare-select chain of
// obs_column_ops_kernel, never a run-time subscript.  A SCALAR is one load of element 0 of its one-element column per row (every lane
// the same address).  Stores are plain vector stores; no __restrict__, since out[t] may be any in[.].
#include "atx_obs_rows.hpp"

namespace atx {

__device__ __forceinline__ double row_flag(bool c) { return c ? 1.0 : 0.0; }

__device__ __forceinline__ double row_op(int op, double x, double y) {
    switch (op) {
        case ATX_COLOP_IS_NAN: return row_flag(x != x);
        case ATX_COLOP_NOT: return row_flag(x == 0.0);
        case ATX_COLOP_CMP_GT: return row_flag(x > y);
        case ATX_COLOP_CMP_LT: return row_flag(x < y);
        case ATX_COLOP_CMP_EQ: return row_flag(x == y);
        case ATX_COLOP_CMP_NE: return row_flag(x != y);
        case ATX_COLOP_CMP_GE: return row_flag(x >= y);
        case ATX_COLOP_CMP_LE: return row_flag(x <= y);
        case ATX_COLOP_ABS_GT: return row_flag(fabs(x) > y);
        case ATX_COLOP_AND: return row_flag(x != 0.0 && y != 0.0);
        case ATX_COLOP_OR: return row_flag(x != 0.0 || y != 0.0);
        case ATX_COLOP_NAN_WHERE: return y != 0.0 ? __longlong_as_double(0x7ff8000000000000ll) : x;
        case ATX_COLOP_CLIP_LOW: return x < y ? y : x;
        case ATX_COLOP_CLIP_HIGH: return x > y ? y : x;
        case ATX_COLOP_FILL_NAN: return x != x ? y : x;
        default: return x;  // SCALAR, COPY: the bits as they are
    }
}

// No __restrict__: out[t] may be any in[.] (in place).  A lane's load of a column comes before its store to it in program order, and no
// other lane touches its row.
__global__ void __launch_bounds__(kBlock) obs_row_program_kernel(const ColumnProgram p, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        double r[ATX_MAX_COLUMN_OPS];
        double y = 0.0;  // the result of the operation before: the host refuses a binary operation at slot 0
        for (int t = 0; t < ATX_MAX_COLUMN_OPS; ++t) {
            if (t >= p.n_ops) break;
            const int op = p.op[t];
            const int s = p.src[t];
            double x;
            if (t == 0 || s < 0) {
                x = p.in[t][op == ATX_COLOP_SCALAR ? 0 : i];
            } else {
                x = r[0];
                for (int u = 1; u < t; ++u) x = (s == u) ? r[u] : x;
            }
            y = row_op(op, x, y);
            r[t] = y;
            if (p.out[t]) p.out[t][i] = y;
        }
    }
}

int launch_obs_row_program(const ColumnProgram& p, int64_t n, hipStream_t stream) {
    hipLaunchKernelGGL(obs_row_program_kernel, dim3(row_grid(n)), dim3(kBlock), 0, stream, p, n);
    ATX_LAUNCH_CHECK("obs_row_program");
    return ATX_OK;
}

}  // namespace atx
