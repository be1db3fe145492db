// Missing station altitudes from an orography: atx_obs_fill_heights.  float64 rows in, float64 out, one lane per row.
//
// The reference's fill_orography filter (R: filters/tabular/fill_heights.py:68-91) selects the rows whose station altitude is NaN or the
// sentinel 9999.0 and hands their coordinates to get_heights (R: filters/tabular/support/utils.py:24-55): one cKDTree per orography axis,
// one nearest-entry query per axis and row, and heights[(lat_idxs, lon_idxs)].  A 1-D cKDTree query is the arg-min of the float64 square
// (a - q) * (a - q) over the axis entries, so it is restated here as a lower-bound search on the axis SORTED ASCENDING (the host sorts
// once and passes the permutation back to file order; descending and shuffled files are then nothing special) followed by the squares of
// the two entries around the query.  The square is monotone in |a - q|, so the smaller of the two is the axis' minimum.  Longitudes do
// not wrap: 359.9 against an axis 0 .. 359 gives 359 — the reference's behaviour, kept.  tests/fill_heights_restatement.py holds the same
// statement in numpy and scipy.
//
// Ties.  Which of two EQUALLY near entries cKDTree returns is an artefact of its build, so the kernel does not decide it: where the square
// of either sorted neighbour of the winner equals the winner's (an exact midpoint, squares that round or underflow to the same value, or
// overflow to infinity), the row's flag gets the axis' bit and the host answers that axis again with cKDTree itself, as interp.device_knn
// does for the k-NN kernel.  Where no neighbour is equal the winner's square is strictly the smallest of the axis, and the index is
// cKDTree's whatever its build.
//
// Launch shape, as atx_obs_rowops.hip and atx_healpix.hip: one row per lane, 256-lane workgroups, a grid-stride loop under a grid cap (kFhGrid), the
// three counters by wave shuffle and one atomic per wave and counter.  A kept row copies its altitude bit for bit and searches nothing; a
// row to fill runs two searches of at most 31 steps over axes of a few KB (they stay in cache) and one gather from heights.  The
// divergence between kept and filled rows is inherent.  The subtraction and the product are separate roundings (-ffp-contract=off).
#include "atx_common.hpp"

namespace atx {

// Grid cap: 2048 workgroups are the 8 waves per SIMD this kernel is resident with on 256 CUs; beyond 2^19 rows a lane takes further
// rows.  Unlike the bad-row counters of the other per-row kernels, `filled` is non-zero in every wave, and atomics on ONE address are
// served one after the other: with a workgroup per 256 rows, 10^7 rows took 1.9 ms whatever they did (156 250 atomics); under this
// cap they are 8192 and out of the way (profiles/fill_heights_bench.json).
constexpr int kFhGrid = 2048;

struct AxisHit {
    int at;    // position in the sorted axis of the entry with the smallest square
    bool tie;  // a sorted neighbour of it has the same square
};

// The entry of the ascending axis[0 .. n) nearest to the finite q by cKDTree's measure, (a - q) * (a - q) in float64.
__device__ __forceinline__ AxisHit nearest_on_axis(const double* __restrict__ axis, int n, double q) {
    int lo = 0, hi = n;  // lower bound: the first position whose entry is >= q
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (axis[mid] < q) lo = mid + 1;
        else hi = mid;
    }
    auto square = [&](int p) {
        const double d = axis[p] - q;
        return d * d;
    };
    int at = lo < n ? lo : n - 1;  // beyond the upper end: the end
    double best = square(at);
    if (lo > 0 && lo < n) {
        const double below = square(lo - 1);
        if (below < best) {
            best = below;
            at = lo - 1;
        }
    }
    const bool tie = (at > 0 && square(at - 1) == best) || (at + 1 < n && square(at + 1) == best);
    return {at, tie};
}

template <typename H>
__global__ void __launch_bounds__(kBlock)
obs_fill_heights_kernel(const double* __restrict__ latitude, const double* __restrict__ longitude, const double* __restrict__ altitude, int64_t n,
                        const double* __restrict__ lat_axis, const int32_t* __restrict__ lat_perm, int n_lat,
                        const double* __restrict__ lon_axis, const int32_t* __restrict__ lon_perm, int n_lon,
                        const H* __restrict__ heights, int64_t pitch, double* __restrict__ out, uint8_t* __restrict__ flags,
                        unsigned long long* counters) {
    unsigned long long filled = 0, flagged = 0, bad = 0;
    for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += (int64_t)gridDim.x * kBlock) {
        const double alt = altitude[r];
        if (!(alt != alt || alt == 9999.0)) {  // R: fill_heights.py:80 — every other row keeps its bits
            out[r] = alt;
            flags[r] = 0;
            continue;
        }
        const double lat = latitude[r], lon = longitude[r];
        // cKDTree refuses a query that is not finite; fabs(x) < inf is false for NaN and +-inf
        if (!(fabs(lat) < __builtin_huge_val()) || !(fabs(lon) < __builtin_huge_val())) {
            out[r] = __builtin_nan("");
            flags[r] = 0;
            bad += 1;
            continue;
        }
        const AxisHit i = nearest_on_axis(lat_axis, n_lat, lat);
        const AxisHit j = nearest_on_axis(lon_axis, n_lon, lon);
        // file-order indices; 64-bit: i * pitch + j passes 2^31 for a 30-arc-second grid
        out[r] = (double)heights[(int64_t)lat_perm[i.at] * pitch + (int64_t)lon_perm[j.at]];
        const uint8_t f = (uint8_t)((i.tie ? ATX_FILL_TIE_LATITUDE : 0) | (j.tie ? ATX_FILL_TIE_LONGITUDE : 0));
        flags[r] = f;
        filled += 1;
        flagged += f ? 1 : 0;
    }
    // wavefront (64-lane) shuffle reduction, then one atomic per wave and counter
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        filled += __shfl_down(filled, off, kWave);
        flagged += __shfl_down(flagged, off, kWave);
        bad += __shfl_down(bad, off, kWave);
    }
    if ((threadIdx.x & (kWave - 1)) == 0) {
        if (filled) atomicAdd(counters + 0, filled);
        if (flagged) atomicAdd(counters + 1, flagged);
        if (bad) atomicAdd(counters + 2, bad);
    }
}

}  // namespace atx

using namespace atx;

extern "C" int atx_obs_fill_heights(const double* latitude, const double* longitude, const double* altitude, int64_t n, const double* lat_axis,
                                    const int32_t* lat_perm, int64_t n_lat, const double* lon_axis, const int32_t* lon_perm, int64_t n_lon,
                                    const void* heights, int64_t heights_pitch, int dtype, double* out, uint8_t* flags, int64_t* counters,
                                    void* stream) {
    ATX_REQUIRE(n >= 0, ATX_EINVAL, "atx_obs_fill_heights: %lld rows", (long long)n);
    ATX_REQUIRE(n_lat >= 1 && n_lon >= 1 && n_lat <= INT32_MAX && n_lon <= INT32_MAX, ATX_EINVAL,
                "atx_obs_fill_heights: an orography of %lld x %lld points (each axis needs 1 .. 2^31 - 1 entries)", (long long)n_lat, (long long)n_lon);
    ATX_REQUIRE(heights_pitch >= n_lon, ATX_ESHAPE, "atx_obs_fill_heights: heights_pitch %lld < n_lon %lld", (long long)heights_pitch,
                (long long)n_lon);
    ATX_REQUIRE(dtype == ATX_F32 || dtype == ATX_F64, ATX_EINVAL, "atx_obs_fill_heights: dtype %d (0: float32, 1: float64)", dtype);
    ATX_REQUIRE(counters, ATX_EINVAL, "atx_obs_fill_heights: null counters");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int st = hip_status(hipMemsetAsync(counters, 0, 3 * sizeof(int64_t), s), "atx_obs_fill_heights memset");
    if (st != ATX_OK) return st;
    if (n == 0) return ATX_OK;
    ATX_REQUIRE(latitude && longitude && altitude && lat_axis && lat_perm && lon_axis && lon_perm && heights && out && flags, ATX_EINVAL,
                "atx_obs_fill_heights: null pointer");
    const dim3 grid(grid_for(n, kBlock, kFhGrid));
    unsigned long long* c = reinterpret_cast<unsigned long long*>(counters);
    if (dtype == ATX_F32)
        hipLaunchKernelGGL(obs_fill_heights_kernel<float>, grid, dim3(kBlock), 0, s, latitude, longitude, altitude, n, lat_axis, lat_perm, (int)n_lat,
                           lon_axis, lon_perm, (int)n_lon, static_cast<const float*>(heights), heights_pitch, out, flags, c);
    else
        hipLaunchKernelGGL(obs_fill_heights_kernel<double>, grid, dim3(kBlock), 0, s, latitude, longitude, altitude, n, lat_axis, lat_perm, (int)n_lat,
                           lon_axis, lon_perm, (int)n_lon, static_cast<const double*>(heights), heights_pitch, out, flags, c);
    ATX_LAUNCH_CHECK("obs_fill_heights");
    return ATX_OK;
}
