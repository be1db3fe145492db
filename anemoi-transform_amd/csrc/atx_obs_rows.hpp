// What the per-row observation kernels share (atx_obs_rowops.hip, atx_obs_column_ops.hip): numpy's degree factors, the cos / sin of a
// row, the grid cap of a one-lane-per-row launch.
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

static unsigned row_grid(int64_t n) {
    const int64_t blocks = (n + kBlock - 1) / kBlock;
    return (unsigned)(blocks < kRowGrid ? blocks : kRowGrid);
}

}  // namespace atx
