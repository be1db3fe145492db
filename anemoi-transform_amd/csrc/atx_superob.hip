// superob: per-group means of an observation table, by pandas' rule, and the nearest row of every group.
//
// superob (R: filters/tabular/superob.py:60-97) thins a table to one row per grid cell, time slot and report type:
// `df.groupby(keys, sort=False)[cols].mean()` for the value columns and `groupby(keys)["distance"].idxmin()` for the row whose
// other columns are kept.  pandas' group mean is ONE compensated (Kahan) sum per group and column, taken in the ROW ORDER of the
// table, NaN skipped, divided by the number of rows that were not NaN (pandas/_libs/groupby.pyx, group_mean):
//
//   y = v - comp;  t = sum + y;  comp = (t - sum) - y;  if (comp != comp) comp = 0;  sum = t;        mean = sum / n
//
// Its bits depend on the order of the rows, so the sum is never split or reordered here: a group is summed front to back, as
// pandas sums it.  (This file is compiled with -ffp-contract=off like the others: the four statements stay four roundings.)
//
// The caller hands over the rows in group order: `order` (row indices, the rows of group g at order[offsets[g] .. offsets[g+1]),
// ascending within a group: a STABLE sort of the rows by group) and `offsets`.  The parallelism is across groups and columns:
//   lane = one group (blockIdx.x * kBlock + threadIdx.x), blockIdx.y = one column.  Typical tables hold millions of groups of
//   1-50 rows.  A lane walks its rows kUnroll at a time: the kUnroll row indices, then the kUnroll values (independent 8-byte
//   gathers, in flight together), then the kUnroll dependent Kahan steps.
//   A group of kLongGroup rows or more is not left to one lane: after the lanes of a wave have finished their short groups, the
//   wave takes its long groups one by one, loads 64 rows at a time (one per lane) and EVERY lane runs the same Kahan chain over
//   the 64 values in row order (a broadcast per value); the result is the sequential sum, bit for bit, with the gathers of a
//   whole wave behind it instead of one lane's.  The chain itself stays sequential by definition: a single group of 10^6 rows
//   costs 10^6 dependent steps of four float64 additions whatever loads them.
// Row indices are compared against [0, n_obs) and segment bounds against [0, n_sel] BEFORE they become addresses; a group whose
// bounds are out of range or not monotone gives NaN / count 0 / nearest -1.  No atomics: every output has one writer.
//
// atx_obs_group_argmin is the same walk with a minimum: the first row of the group with the smallest distance (strict `<` in row
// order = pandas' idxmin on a table in row order), NaN distances never chosen unless the group has nothing else.
#include "atx_common.hpp"

namespace atx {

constexpr int kSuperobUnroll = 8;
constexpr int64_t kLongGroup = 256;  // rows from which a group is summed by its wave rather than by its lane (not yet tuned on the GPU)

struct Kahan {
    double sum = 0.0, comp = 0.0;
    int64_t n = 0;
    __device__ __forceinline__ void add(double v) {
        if (v != v) return;  // NaN rows do not take part
        const double y = v - comp;
        const double t = sum + y;
        comp = (t - sum) - y;
        if (comp != comp) comp = 0.0;  // inf - inf: pandas resets the compensation
        sum = t;
        ++n;
    }
};

__device__ __forceinline__ double superob_value(const double* __restrict__ col, const int32_t* __restrict__ order, int64_t k, int64_t n_obs) {
    const int64_t r = order[k];
    return (r >= 0 && r < n_obs) ? col[r] : quiet_nan<double>();  // never an address outside the column
}

__device__ __forceinline__ bool superob_segment(const int64_t* __restrict__ offsets, int64_t g, int64_t n_groups, int64_t n_sel, int64_t& beg,
                                                int64_t& end) {
    beg = end = 0;
    if (g >= n_groups) return false;
    const int64_t b = offsets[g], e = offsets[g + 1];
    if (b < 0 || e < b || e > n_sel) return false;
    beg = b;
    end = e;
    return true;
}

__global__ void __launch_bounds__(kBlock)
obs_group_mean_kernel(const double* __restrict__ values, int64_t n_obs, int64_t val_pitch, const int32_t* __restrict__ order, int64_t n_sel,
                      const int64_t* __restrict__ offsets, int64_t n_groups, double* __restrict__ mean, int64_t* __restrict__ count,
                      int64_t out_pitch) {
    const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int c = blockIdx.y;
    const int lane = threadIdx.x & (kWave - 1);
    const double* __restrict__ col = values + (int64_t)c * val_pitch;
    int64_t beg, end;
    const bool ok = superob_segment(offsets, g, n_groups, n_sel, beg, end);
    const bool is_long = ok && end - beg >= kLongGroup;
    Kahan acc;
    if (ok && !is_long) {
        int64_t k = beg;
        for (; k + kSuperobUnroll <= end; k += kSuperobUnroll) {
            double v[kSuperobUnroll];
#pragma unroll
            for (int j = 0; j < kSuperobUnroll; ++j) v[j] = superob_value(col, order, k + j, n_obs);
#pragma unroll
            for (int j = 0; j < kSuperobUnroll; ++j) acc.add(v[j]);
        }
        for (; k < end; ++k) acc.add(superob_value(col, order, k, n_obs));
    }
    // the long groups of this wave, one after the other, every lane running the same chain (no lane has left: all 64 take part)
    unsigned long long todo = __ballot(is_long);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int64_t b = __shfl(beg, src, kWave), e = __shfl(end, src, kWave);
        Kahan wide;
        double next = b + lane < e ? superob_value(col, order, b + lane, n_obs) : quiet_nan<double>();
        for (int64_t k0 = b; k0 < e; k0 += kWave) {
            const double mine = next;
            const int64_t kn = k0 + kWave + lane;
            next = kn < e ? superob_value(col, order, kn, n_obs) : quiet_nan<double>();  // in flight during the chain below
#pragma unroll
            for (int j = 0; j < kWave; ++j) wide.add(__shfl(mine, j, kWave));  // rows past the end were loaded as NaN: skipped
        }
        if (lane == src) acc = wide;
    }
    if (g < n_groups) {
        mean[(int64_t)c * out_pitch + g] = acc.n > 0 ? acc.sum / (double)acc.n : quiet_nan<double>();
        count[(int64_t)c * out_pitch + g] = acc.n;
    }
}

struct Nearest {
    double d = __longlong_as_double(0x7ff0000000000000ll);  // +inf
    int64_t k = INT64_MAX;                                  // position in `order`; INT64_MAX: nothing yet
    __device__ __forceinline__ void see(double v, int64_t at) {
        if (v < d || (k == INT64_MAX && v == v)) {  // strict: the first of equals stays (a first +inf is taken too)
            d = v;
            k = at;
        }
    }
    __device__ __forceinline__ void merge(double od, int64_t ok) {
        if (od < d || (od == d && ok < k)) {
            d = od;
            k = ok;
        }
    }
};

__global__ void __launch_bounds__(kBlock)
obs_group_argmin_kernel(const double* __restrict__ distance, int64_t n_obs, const int32_t* __restrict__ order, int64_t n_sel,
                        const int64_t* __restrict__ offsets, int64_t n_groups, int32_t* __restrict__ nearest) {
    const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    int64_t beg, end;
    const bool ok = superob_segment(offsets, g, n_groups, n_sel, beg, end);
    const bool is_long = ok && end - beg >= kLongGroup;
    Nearest best;
    if (ok && !is_long) {
        int64_t k = beg;
        for (; k + kSuperobUnroll <= end; k += kSuperobUnroll) {
            double v[kSuperobUnroll];
#pragma unroll
            for (int j = 0; j < kSuperobUnroll; ++j) v[j] = superob_value(distance, order, k + j, n_obs);
#pragma unroll
            for (int j = 0; j < kSuperobUnroll; ++j) best.see(v[j], k + j);
        }
        for (; k < end; ++k) best.see(superob_value(distance, order, k, n_obs), k);
    }
    // a minimum may be taken in any order as long as equals are settled by position: lanes take every 64th row, then meet
    unsigned long long todo = __ballot(is_long);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int64_t b = __shfl(beg, src, kWave), e = __shfl(end, src, kWave);
        Nearest wide;
        for (int64_t k = b + lane; k < e; k += kWave) wide.see(superob_value(distance, order, k, n_obs), k);
#pragma unroll
        for (int m = kWave / 2; m > 0; m >>= 1) {
            const double od = __shfl_xor(wide.d, m, kWave);
            const int64_t ok2 = __shfl_xor(wide.k, m, kWave);
            wide.merge(od, ok2);
        }
        if (lane == src) best = wide;
    }
    if (g < n_groups) {
        int64_t at = best.k != INT64_MAX ? best.k : (ok && end > beg ? beg : -1);  // every distance NaN: the group's first row
        int64_t r = at >= 0 ? (int64_t)order[at] : -1;
        nearest[g] = (r >= 0 && r < n_obs) ? (int32_t)r : -1;
    }
}

static int superob_sizes(const char* fn, int64_t n_obs, int64_t n_sel, int64_t n_groups) {
    ATX_REQUIRE(n_obs >= 0 && n_sel >= 0 && n_groups >= 0, ATX_EINVAL, "%s: bad sizes", fn);
    ATX_REQUIRE(n_obs < 0x80000000ll, ATX_EINVAL, "%s: %lld rows do not fit an int32 row index", fn, (long long)n_obs);
    ATX_REQUIRE(n_sel <= n_obs, ATX_ESHAPE, "%s: %lld rows in group order, the table has %lld", fn, (long long)n_sel, (long long)n_obs);
    ATX_REQUIRE(n_groups <= n_sel, ATX_ESHAPE, "%s: %lld groups of %lld rows (a group has at least one row)", fn, (long long)n_groups,
                (long long)n_sel);
    return ATX_OK;
}

}  // namespace atx

using namespace atx;

extern "C" int atx_obs_group_mean(const double* values, int64_t n_obs, int32_t n_cols, int64_t val_pitch, const int32_t* order, int64_t n_sel,
                                  const int64_t* offsets, int64_t n_groups, double* mean, int64_t* count, int64_t out_pitch, void* stream) {
    ATX_REQUIRE(n_cols > 0 && n_cols <= 65535, ATX_EINVAL, "atx_obs_group_mean: 1 .. 65535 columns, got %d", (int)n_cols);
    int st = superob_sizes("atx_obs_group_mean", n_obs, n_sel, n_groups);
    if (st != ATX_OK) return st;
    ATX_REQUIRE(val_pitch >= n_obs, ATX_ESHAPE, "atx_obs_group_mean: val_pitch %lld below n_obs", (long long)val_pitch);
    ATX_REQUIRE(out_pitch >= n_groups, ATX_ESHAPE, "atx_obs_group_mean: out_pitch %lld below n_groups", (long long)out_pitch);
    if (n_groups == 0) return ATX_OK;
    ATX_REQUIRE(values && order && offsets && mean && count, ATX_EINVAL, "atx_obs_group_mean: null pointer");
    const dim3 grid((unsigned)((n_groups + kBlock - 1) / kBlock), (unsigned)n_cols);
    hipLaunchKernelGGL(obs_group_mean_kernel, grid, dim3(kBlock), 0, static_cast<hipStream_t>(stream), values, n_obs, val_pitch, order, n_sel,
                       offsets, n_groups, mean, count, out_pitch);
    ATX_LAUNCH_CHECK("obs_group_mean");
    return ATX_OK;
}

extern "C" int atx_obs_group_argmin(const double* distance, int64_t n_obs, const int32_t* order, int64_t n_sel, const int64_t* offsets,
                                    int64_t n_groups, int32_t* nearest, void* stream) {
    int st = superob_sizes("atx_obs_group_argmin", n_obs, n_sel, n_groups);
    if (st != ATX_OK) return st;
    if (n_groups == 0) return ATX_OK;
    ATX_REQUIRE(distance && order && offsets && nearest, ATX_EINVAL, "atx_obs_group_argmin: null pointer");
    const dim3 grid((unsigned)((n_groups + kBlock - 1) / kBlock));
    hipLaunchKernelGGL(obs_group_argmin_kernel, grid, dim3(kBlock), 0, static_cast<hipStream_t>(stream), distance, n_obs, order, n_sel, offsets,
                       n_groups, nearest);
    ATX_LAUNCH_CHECK("obs_group_argmin");
    return ATX_OK;
}
