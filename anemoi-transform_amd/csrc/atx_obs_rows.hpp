// What the per-row observation kernels share (atx_obs_rowops.hip, atx_obs_column_ops.hip, atx_obs_row_program.hip,
// atx_obs_row_expr.hip): numpy's degree factors, the cos / sin of a row, the grid cap of a one-lane-per-row launch, and the program that
// atx_obs_column_ops hands to either of its two kernels.
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

static unsigned row_grid(int64_t n) { return grid_for(n, kBlock, kRowGrid); }

}  // namespace atx
