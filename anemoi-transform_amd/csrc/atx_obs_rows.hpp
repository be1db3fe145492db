// What the per-row observation kernels share (atx_obs_rowops.hip, atx_obs_column_ops.hip, atx_obs_row_program.hip,
// atx_obs_row_expr.hip): numpy's degree factors, the cos / sin of a row, the grid cap of a one-lane-per-row launch, the program that
// atx_obs_column_ops hands to either of its two kernels, and the postfix program of the row-expression kernel.
#pragma once

#include "atx_common.hpp"

namespace atx {

constexpr double kPi = 3.141592653589793;  // np.pi
constexpr double kRad = kPi / 180.0;       // np.deg2rad / np.radians: x * (pi / 180)
constexpr double kDeg = 180.0 / kPi;       // np.degrees: x * (180 / pi)
constexpr int kRowGrid = 1 << 20;          // grid cap: 2^28 rows before a lane takes a second one

__device__ __forceinline__ void row_sincos(double x, double& sn, double& cs) {
    if (!sincos_moderate(x, sn, cs)) sincos(x, &sn, &cs);  // |x| >= 1e5, infinite, NaN
}

// The program of one atx_obs_column_ops call, by value in the kernel arguments: no table on the device, no copy.
struct ColumnProgram {
    const double* in[ATX_MAX_COLUMN_OPS];
    double* out[ATX_MAX_COLUMN_OPS];
    int32_t op[ATX_MAX_COLUMN_OPS];  // dwords: a scalar load can fetch them at a run-time index, a byte needs a vector load
    int32_t src[ATX_MAX_COLUMN_OPS];
    int32_t n_ops;
};

// atx_obs_row_program.hip: the launch of a program of codes >= ATX_COLOP_SCALAR (validated by atx_obs_column_ops, n > 0)
int launch_obs_row_program(const ColumnProgram& p, int64_t n, hipStream_t stream);

// The program of one row-expression launch, by value in the kernel arguments (about 1.1 KB).  Everything indexed at run time is dwords
// or qwords, so a scalar load fetches it.
struct ExprProgram {
    const double* in[ATX_EXPR_MAX_INPUTS];
    double* out[ATX_EXPR_MAX_RESULTS];
    double consts[ATX_EXPR_MAX_CONSTS];
    int32_t code[ATX_EXPR_MAX_INSTR];
    int32_t arg0[ATX_EXPR_MAX_INSTR];
    int32_t arg1[ATX_EXPR_MAX_INSTR];
    int32_t n_instr;
    int32_t n_results;
    unsigned long long* keep_words;  // with its chunk_counts, or both null
    int64_t* chunk_counts;
};

// atx_api.hip: a flat row-expression program and a keep-positions call, validated (stack depth simulated) and launched.  Reached from
// atx_obs_column_ops, which reads them out of the slots of its third family of codes.
int obs_row_expr_call(int32_t n_instr, const int32_t* code, const int32_t* arg0, const int32_t* arg1, int32_t n_inputs, const double* const* in,
                      int32_t n_consts, const double* consts, int32_t n_results, double* const* out, bool keep, uint64_t* keep_words,
                      int64_t* chunk_counts, int64_t n, void* stream);
int obs_keep_positions_call(const uint64_t* words, const int64_t* chunk_offsets, int64_t n, int64_t* positions, int64_t n_positions, void* stream);

// atx_obs_row_expr.hip: the launches behind them (n > 0)
int launch_obs_row_expr(const ExprProgram& p, int64_t n, hipStream_t stream);
int launch_obs_keep_positions(const unsigned long long* words, const int64_t* chunk_offsets, int64_t n, int64_t* positions, int64_t n_positions,
                              hipStream_t stream);

static unsigned row_grid(int64_t n) {
    const int64_t blocks = (n + kBlock - 1) / kBlock;
    return (unsigned)(blocks < kRowGrid ? blocks : kRowGrid);
}

}  // namespace atx
