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

#include <functional>

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

// The third family: a postfix row-expression program, its results and its keep rows, or a keep-positions call, written as slots
// (include/atx.h).  The slots are read into the flat program that obs_row_expr_call validates: columns by their pointers (one input per
// distinct pointer), constants by value from the HOST doubles in[t] points to.
static int expr_slots(int32_t n_ops, const int32_t* op, const int32_t* src, const double* const* in, double* const* out, int64_t n, void* stream) {
    ATX_REQUIRE(n_ops <= ATX_EXPR_MAX_SLOTS, ATX_EINVAL, "atx_obs_column_ops, row expression: 1 .. %d slots, got %d", ATX_EXPR_MAX_SLOTS, (int)n_ops);
    ATX_REQUIRE(src && in && out, ATX_EINVAL, "atx_obs_column_ops: null program array");
    if (op[0] == ATX_COLOP_KEEP_POSITIONS) {
        ATX_REQUIRE(n_ops == 2 && op[1] == ATX_COLOP_KEEP_OFFSETS && src[0] >= 0 && src[1] >= 0, ATX_EINVAL,
                    "atx_obs_column_ops, keep positions: two slots, KEEP_POSITIONS and KEEP_OFFSETS, with the capacity in src, not negative");
        return obs_keep_positions_call(reinterpret_cast<const uint64_t*>(in[0]), reinterpret_cast<const int64_t*>(in[1]), n,
                                       reinterpret_cast<int64_t*>(out[0]), (int64_t)src[0] + ((int64_t)src[1] << 31), stream);
    }
    int32_t code[ATX_EXPR_MAX_INSTR], arg0[ATX_EXPR_MAX_INSTR], arg1[ATX_EXPR_MAX_INSTR];
    const double* cols[ATX_EXPR_MAX_INPUTS];
    double consts[ATX_EXPR_MAX_CONSTS];
    double* outs[ATX_EXPR_MAX_RESULTS];
    int n_instr = 0, n_in = 0, n_consts = 0, n_results = 0;
    // The constants first: the host ranges the PUSH_CONST and IN_SET slots point to, merged where they overlap or touch (slices of one
    // table are held once), copied in address order.
    const double* lo[ATX_EXPR_MAX_SLOTS];
    const double* hi[ATX_EXPR_MAX_SLOTS];
    int where[ATX_EXPR_MAX_SLOTS];
    int n_ranges = 0;
    for (int t = 0; t < n_ops; ++t) {
        const int e = op[t] - ATX_COLOP_EXPR;
        if (e != ATX_EXPR_PUSH_CONST && e != ATX_EXPR_IN_SET) continue;
        const int count = e == ATX_EXPR_IN_SET ? src[t] : 1;
        ATX_REQUIRE(in[t] && count >= 1, ATX_EINVAL, "atx_obs_column_ops, row expression: slot %d: a constant or IN_SET slot points to %d host doubles", t,
                    count);
        int k = n_ranges++;
        for (; k > 0 && std::less<const double*>()(in[t], lo[k - 1]); --k) {
            lo[k] = lo[k - 1];
            hi[k] = hi[k - 1];
        }
        lo[k] = in[t];
        hi[k] = in[t] + count;
    }
    int n_merged = 0;
    for (int k = 0; k < n_ranges; ++k) {
        if (n_merged > 0 && !std::less<const double*>()(hi[n_merged - 1], lo[k])) {
            if (std::less<const double*>()(hi[n_merged - 1], hi[k])) hi[n_merged - 1] = hi[k];
        } else {
            lo[n_merged] = lo[k];
            hi[n_merged++] = hi[k];
        }
    }
    for (int k = 0; k < n_merged; ++k) {
        where[k] = n_consts;
        ATX_REQUIRE(hi[k] - lo[k] <= ATX_EXPR_MAX_CONSTS - n_consts, ATX_EINVAL, "atx_obs_column_ops, row expression: 0 .. %d constants", ATX_EXPR_MAX_CONSTS);
        for (const double* c = lo[k]; c != hi[k]; ++c) consts[n_consts++] = *c;
    }
    bool keep = false;
    uint64_t* words = nullptr;
    int64_t* counts = nullptr;
    for (int t = 0; t < n_ops; ++t) {
        ATX_REQUIRE(!keep, ATX_EINVAL, "atx_obs_column_ops, row expression: slot %d follows the KEEP slot, which is the last", t);
        if (op[t] == ATX_COLOP_EXPR_RESULT) {
            ATX_REQUIRE(n_results < ATX_EXPR_MAX_RESULTS, ATX_EINVAL, "atx_obs_column_ops, row expression: 0 .. %d value results", ATX_EXPR_MAX_RESULTS);
            ATX_REQUIRE(src[t] == n_results, ATX_EINVAL, "atx_obs_column_ops, row expression: RESULT slots name the stack slots 0, 1, .. in order, got %d",
                        (int)src[t]);
            outs[n_results++] = out[t];
            continue;
        }
        if (op[t] == ATX_COLOP_EXPR_KEEP) {
            keep = true;
            words = reinterpret_cast<uint64_t*>(out[t]);
            counts = reinterpret_cast<int64_t*>(const_cast<double*>(in[t]));
            continue;
        }
        const int e = op[t] - ATX_COLOP_EXPR;
        ATX_REQUIRE(e >= ATX_EXPR_PUSH_COL && e <= ATX_EXPR_NAN_WHERE, ATX_EINVAL, "atx_obs_column_ops, row expression: slot %d has the unknown code %d", t,
                    (int)op[t]);
        ATX_REQUIRE(n_results == 0, ATX_EINVAL, "atx_obs_column_ops, row expression: instruction slot %d follows a RESULT slot", t);
        ATX_REQUIRE(n_instr < ATX_EXPR_MAX_INSTR, ATX_EINVAL, "atx_obs_column_ops, row expression: 1 .. %d instructions", ATX_EXPR_MAX_INSTR);
        int a0 = src[t], a1 = 0;
        if (e == ATX_EXPR_PUSH_COL) {
            ATX_REQUIRE(in[t] || n == 0, ATX_EINVAL, "atx_obs_column_ops, row expression: slot %d pushes a null input column", t);
            for (a0 = 0; a0 < n_in && cols[a0] != in[t]; ++a0) {
            }
            if (a0 == n_in) {
                ATX_REQUIRE(n_in < ATX_EXPR_MAX_INPUTS, ATX_EINVAL, "atx_obs_column_ops, row expression: 0 .. %d input columns", ATX_EXPR_MAX_INPUTS);
                cols[n_in++] = in[t];
            }
        } else if (e == ATX_EXPR_PUSH_CONST || e == ATX_EXPR_IN_SET) {
            int k = 0;  // the merged range that holds this slot's
            while (std::less<const double*>()(in[t], lo[k]) || !std::less<const double*>()(in[t], hi[k])) ++k;
            a0 = where[k] + (int)(in[t] - lo[k]);
            a1 = e == ATX_EXPR_IN_SET ? src[t] : 0;
        }
        code[n_instr] = e;
        arg0[n_instr] = a0;
        arg1[n_instr++] = a1;
    }
    return obs_row_expr_call(n_instr, code, arg0, arg1, n_in, cols, n_consts, consts, n_results, outs, keep, words, counts, n, stream);
}

extern "C" int atx_obs_column_ops(int32_t n_ops, const int32_t* op, const int32_t* src, const double* const* in, double* const* out, int64_t n,
                                  void* stream) {
    ATX_REQUIRE(n >= 0, ATX_EINVAL, "atx_obs_column_ops: %lld rows", (long long)n);
    if (op && n_ops >= 1 && op[0] >= ATX_COLOP_EXPR) return expr_slots(n_ops, op, src, in, out, n, static_cast<hipStream_t>(stream));
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
