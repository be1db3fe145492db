// apply_column_transformations: a program of single-input library functions over float64 columns, one launch.
//
// The reference (R: filters/tabular/apply_column_transformations.py:18-61, :132-138) applies its transformations one after the other,
// each a numpy ufunc over a whole column of the DataFrame, so a later one sees an earlier one's result.  Here a run of up to
// ATX_MAX_COLUMN_OPS of them is ONE pass over the rows: operation t reads its column from memory (src[t] < 0) or takes the result of an
// earlier operation of the same row from a register (src[t] = s < t), and stores its own result unless a later operation replaces it
// (out[t] == NULL).  The program travels in the kernel arguments: no table on the device, no copy.
//
// Numerics, in the source's operation order and without contraction: log and safe_log are atx_log (safe_log of the
// float64 sum x + 1e-10), exp is atx_exp, log1p the device library's (its own argument below 2^-54), sqrt correctly rounded, abs clears the sign bit; sin / cos
// are row_sincos — sincos_moderate below 1e5, the device library beyond — of x or of x * (pi / 180), which is np.deg2rad's product.
//
// Launch shape: the per-row kernels' (atx_obs_rowops.hip).  The program is uniform over the launch, so every branch on it is
// scalar and every read of it a scalar load.  The results of a row stay in VGPRs: "the result of operation s" is a compare-select
// chain on the uniform index, never `r[s]` — a run-time subscript would put the array in scratch.  The compiler keeps the loop over
// the operations rolled (ONE copy of the ten functions, 1 143 instructions, where sixteen would not fit the instruction cache; it
// refuses an unroll pragma here, so there is none) and addresses `r[]` through the VGPR index register: 114 VGPRs, no scratch.
// That is this compiler's choice, not something the source can force: tools/kernel_resources.py reads it from the code object and
// tests/test_host_api.py::test_no_streaming_kernel_uses_scratch_memory fails the build that decides otherwise.
//
// The entry point carries a second family of codes, ATX_COLOP_SCALAR and above: the compares, selects and row predicates of the tabular
// QC filters (atx_obs_row_program.hip).  A program is of one family; the check below decides which kernel runs.
#include "atx_obs_rows.hpp"

namespace atx {

__device__ __forceinline__ double column_op(int op, double x) {
    switch (op) {
        case ATX_COLOP_LOG:
        case ATX_COLOP_SAFE_LOG: return atx_log(op == ATX_COLOP_SAFE_LOG ? x + 1e-10 : x);
        // below 2^-54 log1p(x) = x (1 - x / 2 + ...) rounds to x: -0.0 stays -0.0 (the device library answers +0.0) and a subnormal
        // stays itself (the device library is one subnormal step off at 3e-318)
        case ATX_COLOP_LOG1P: return fabs(x) < 0x1p-54 ? x : log1p(x);
        case ATX_COLOP_SQRT: return sqrt(x);
        case ATX_COLOP_EXP: return atx_exp(x);
        case ATX_COLOP_ABS: return fabs(x);
        default: {  // sin, sin_deg, cos, cos_deg
            const bool degrees = op == ATX_COLOP_SIN_DEG || op == ATX_COLOP_COS_DEG;
            double sn, cs;
            row_sincos(degrees ? x * kRad : x, sn, cs);
            return (op == ATX_COLOP_SIN || op == ATX_COLOP_SIN_DEG) ? sn : cs;
        }
    }
}

// No __restrict__: out[t] may be any in[.] (in place).  A lane's load of a column comes before its store to it in program order, and no
// other lane touches its row.
__global__ void __launch_bounds__(kBlock) obs_column_ops_kernel(const ColumnProgram p, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        double r[ATX_MAX_COLUMN_OPS];
        for (int t = 0; t < ATX_MAX_COLUMN_OPS; ++t) {
            if (t >= p.n_ops) break;
            const int s = p.src[t];
            double x;
            if (t == 0 || s < 0) {
                x = p.in[t][i];
            } else {
                x = r[0];
                for (int u = 1; u < t; ++u) x = (s == u) ? r[u] : x;
            }
            r[t] = column_op(p.op[t], x);
            if (p.out[t]) p.out[t][i] = r[t];
        }
    }
}

}  // namespace atx

using namespace atx;

extern "C" int atx_obs_column_ops(int32_t n_ops, const int32_t* op, const int32_t* src, const double* const* in, double* const* out, int64_t n,
                                  void* stream) {
    ATX_REQUIRE(n >= 0, ATX_EINVAL, "atx_obs_column_ops: %lld rows", (long long)n);
    ATX_REQUIRE(n_ops >= 1 && n_ops <= ATX_MAX_COLUMN_OPS, ATX_EINVAL, "atx_obs_column_ops: 1 .. %d operations, got %d", ATX_MAX_COLUMN_OPS,
                (int)n_ops);
    ATX_REQUIRE(op && src && in && out, ATX_EINVAL, "atx_obs_column_ops: null program array");
    ColumnProgram p = {};
    p.n_ops = n_ops;
    const bool rows = op[0] >= ATX_COLOP_SCALAR;  // the family of the program: library functions, or the row operations of the QC filters
    for (int t = 0; t < n_ops; ++t) {
        ATX_REQUIRE((op[t] >= ATX_COLOP_LOG && op[t] <= ATX_COLOP_COS_DEG) || (op[t] >= ATX_COLOP_SCALAR && op[t] <= ATX_COLOP_FILL_NAN), ATX_EINVAL,
                    "atx_obs_column_ops: operation %d has the unknown code %d", t, (int)op[t]);
        ATX_REQUIRE((op[t] >= ATX_COLOP_SCALAR) == rows, ATX_EINVAL,
                    "atx_obs_column_ops: operation %d (code %d) mixes the two families: a program is all codes 0 .. %d or all codes %d .. %d", t,
                    (int)op[t], (int)ATX_COLOP_COS_DEG, (int)ATX_COLOP_SCALAR, (int)ATX_COLOP_FILL_NAN);
        ATX_REQUIRE(src[t] < t, ATX_EINVAL, "atx_obs_column_ops: operation %d takes the result of operation %d, which is not an earlier one", t,
                    (int)src[t]);
        ATX_REQUIRE(op[t] != ATX_COLOP_SCALAR || src[t] < 0, ATX_EINVAL,
                    "atx_obs_column_ops: operation %d is a SCALAR and reads in[%d][0]: its src must be -1, got %d", t, t, (int)src[t]);
        ATX_REQUIRE(op[t] < ATX_COLOP_CMP_GT || t > 0, ATX_EINVAL,
                    "atx_obs_column_ops: operation %d (code %d) is binary: its second operand is the result of the operation before it, and there is none",
                    t, (int)op[t]);
        ATX_REQUIRE(src[t] >= 0 || in[t] || n == 0, ATX_EINVAL, "atx_obs_column_ops: operation %d reads a null column", t);
        p.op[t] = op[t];
        p.src[t] = src[t] < 0 ? -1 : src[t];
        p.in[t] = src[t] < 0 ? in[t] : nullptr;
        p.out[t] = out[t];
    }
    if (n == 0) return ATX_OK;
    if (rows) return launch_obs_row_program(p, n, static_cast<hipStream_t>(stream));
    hipLaunchKernelGGL(obs_column_ops_kernel, dim3(row_grid(n)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), p, n);
    ATX_LAUNCH_CHECK("obs_column_ops");
    return ATX_OK;
}
