// Per-row observation operators: forcings, satellite view angles, brightness temperature.  float64, one lane per row.
//
// Real observation recipes put derived columns between `superob` and `irregular_to_grid`: solar and calendar forcings
// (R: filters/tabular/add_forcings.py, support/compute_forcings.py), viewing geometry (R: add_azimuth.py, add_msg_angles.py,
// support/sat_view_angles.py) and, for CrIS, the inverse Planck law (R: radiance_to_brightness_temperature.py).  In the reference
// they are numpy expressions over the columns of a DataFrame; here each is ONE launch over columns that stay in HBM.
//
// Numerics.  Every statement is evaluated in the operation order of the source, literal for literal, with IEEE
// division and without contraction (-ffp-contract=off), so everything that is pure arithmetic — the calendar, the arguments of the
// trigonometric functions, numpy's `%` — has numpy's bits.  cos / sin of moderate angles are sincos_moderate (atx_common.hpp, < 1 ulp),
// anything else the device library's sincos; asin, acos, atan and log1p are the device library's (2, 2, 2 and 1 ulp in the HIP math
// tables), sqrt is correctly rounded.  tests/test_gpu_obs_rowops.py holds the results against exact arithmetic.
//
// Launch shape.  The kernels are VALU-bound (five to eight float64 sincos per row against 24-80 bytes of traffic), not HBM-bound:
// one row per lane, 256-lane workgroups, a grid-stride loop under a grid cap; consecutive lanes touch consecutive elements of every
// column, and the outputs are rows of one [n_out, pitch] block, so every load and store of a wave is one contiguous 512-byte run.
// Which outputs are wanted is uniform over the launch: the branches on it are scalar.
#include "atx_obs_rows.hpp"

namespace atx {

constexpr int64_t kNaT = INT64_MIN;                    // numpy's / pandas' NaT
constexpr int64_t kNsPerSecond = 1000000000ll;
constexpr int64_t kNsPerDay = 86400ll * kNsPerSecond;

// numpy's float `%`: fmod, then the result takes the sign of the divisor (b > 0 here).
__device__ __forceinline__ double numpy_mod(double a, double b) {
    double m = fmod(a, b);
    if (m != 0.0) {
        if (m < 0.0) m += b;
    } else {
        m = copysign(0.0, b);
    }
    return m;
}

// np.clip(x, lo, hi) of the clip ufunc: min(max(x, lo), hi), a NaN x stays.
__device__ __forceinline__ double numpy_clip(double x, double lo, double hi) {
    x = (x > lo || x != x) ? x : lo;
    return (x < hi || x != x) ? x : hi;
}

// Days since 1970-01-01 of 1 January of the (proleptic Gregorian) year that holds day `z` — civil-from-days for the year, then
// days-from-civil of its first day; integer arithmetic only, negative days included.
__device__ __forceinline__ int64_t year_start_days(int64_t z) {
    z += 719468;  // days from 0000-03-01
    const int64_t era = (z >= 0 ? z : z - 146096) / 146097;
    const int64_t doe = z - era * 146097;                                       // [0, 146096]
    const int64_t yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;  // [0, 399]
    const int64_t doy = doe - (365 * yoe + yoe / 4 - yoe / 100);                // [0, 365], from 1 March
    const int64_t y = yoe + era * 400 + (doy >= 306 ? 1 : 0);                   // January and February belong to the next civil year
    // days_from_civil(y, 1, 1): January counts as month 13 of the year before
    const int64_t yy = y - 1;
    const int64_t era2 = (yy >= 0 ? yy : yy - 399) / 400;
    const int64_t yoe2 = yy - era2 * 400;
    const int64_t doe2 = yoe2 * 365 + yoe2 / 4 - yoe2 / 100 + 306;  // (153 * 10 + 2) / 5 = 306: 1 January, counted from 1 March
    return era2 * 146097 + doe2 - 719468;
}

enum : uint32_t {
    kCosJulianDay = 1u << 0,
    kSinJulianDay = 1u << 1,
    kCosSza = 1u << 2,
    kSinLocalTime = 1u << 3,
    kCosLocalTime = 1u << 4,
    kCosLatitude = 1u << 5,
    kSinLatitude = 1u << 6,
    kCosLongitude = 1u << 7,
    kSinLongitude = 1u << 8,
    kAllForcings = (1u << 9) - 1,
};

__global__ void __launch_bounds__(kBlock)
obs_forcings_kernel(const int64_t* __restrict__ date_ns, const double* __restrict__ latitude, const double* __restrict__ longitude, int64_t n,
                    uint32_t mask, double* __restrict__ out, int64_t pitch) {
    const bool want_date = mask & (kCosJulianDay | kSinJulianDay | kCosSza | kSinLocalTime | kCosLocalTime);
    const bool want_hours = mask & (kCosSza | kSinLocalTime | kCosLocalTime);
    const bool want_angle = mask & (kCosJulianDay | kSinJulianDay | kCosSza);
    const bool want_lat = mask & (kCosSza | kCosLatitude | kSinLatitude);
    const bool want_lon = mask & (kCosSza | kSinLocalTime | kCosLocalTime | kCosLongitude | kSinLongitude);
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const double nan = quiet_nan<double>();
        double julian_day = nan, hours = nan;
        if (want_date) {
            const int64_t ns = date_ns[i];
            if (ns != kNaT) {
                // R: add_forcings.py:99-102, :111-114 — delta.days and delta.seconds are WHOLE days and seconds
                int64_t days = ns / kNsPerDay;
                int64_t rem = ns - days * kNsPerDay;
                if (rem < 0) {  // floor division: dates before 1970
                    rem += kNsPerDay;
                    days -= 1;
                }
                const double seconds = (double)(rem / kNsPerSecond);
                const double day_fraction = seconds / 86400.0;
                julian_day = (double)(days - year_start_days(days)) + day_fraction;
                hours = day_fraction * 24;
            }
        }
        const double lat = want_lat ? latitude[i] : nan;
        const double lon = want_lon ? longitude[i] : nan;
        double* __restrict__ o = out + i;
        double sin_a = nan, cos_a = nan, angle = nan;
        if (want_angle) {
            angle = julian_day / 365.25 * kPi * 2;  // R: add_forcings.py:107, compute_forcings.py:29
            row_sincos(angle, sin_a, cos_a);
        }
        if (mask & kCosJulianDay) {
            *o = cos_a;
            o += pitch;
        }
        if (mask & kSinJulianDay) {
            *o = sin_a;
            o += pitch;
        }
        double sin_lat = nan, cos_lat = nan;
        if (want_lat) row_sincos(lat * kRad, sin_lat, cos_lat);
        if (mask & kCosSza) {
            // R: compute_forcings.py:14-87
            double sin_2a, cos_2a, sin_3a, cos_3a;
            row_sincos(2 * angle, sin_2a, cos_2a);
            row_sincos(3 * angle, sin_3a, cos_3a);
            double declination = 0.396372 - 22.91327 * cos_a + 4.025430 * sin_a - 0.387205 * cos_2a + 0.051967 * sin_2a - 0.154527 * cos_3a +
                                 0.084798 * sin_3a;
            const double time_correction = 0.004297 + 0.107029 * cos_a - 1.837877 * sin_a - 0.837378 * cos_2a - 2.340475 * sin_2a;
            declination = declination * kRad;
            double sin_dec, cos_dec;
            row_sincos(declination, sin_dec, cos_dec);
            const double sindec_sinlat = sin_dec * sin_lat;
            const double cosdec_coslat = cos_dec * cos_lat;
            const double solar_angle = ((hours - 12) * 15 + lon + time_correction) * kRad;
            double sin_sa, cos_sa;
            row_sincos(solar_angle, sin_sa, cos_sa);
            const double zenith = sindec_sinlat + cosdec_coslat * cos_sa;
            *o = (zenith > 0.0 || zenith != zenith) ? zenith : 0.0;  // np.clip(zenith_angle, 0, None)
            o += pitch;
        }
        if (mask & (kSinLocalTime | kCosLocalTime)) {
            // R: add_forcings.py:123-127
            const double local_time = numpy_mod(lon / 360.0 * 24.0 + hours, 24.0);
            double sn, cs;
            row_sincos(local_time / 24 * kPi * 2, sn, cs);
            if (mask & kSinLocalTime) {
                *o = sn;
                o += pitch;
            }
            if (mask & kCosLocalTime) {
                *o = cs;
                o += pitch;
            }
        }
        if (mask & kCosLatitude) {
            *o = cos_lat;
            o += pitch;
        }
        if (mask & kSinLatitude) {
            *o = sin_lat;
            o += pitch;
        }
        if (mask & (kCosLongitude | kSinLongitude)) {
            double sn, cs;
            row_sincos(lon * kRad, sn, cs);
            if (mask & kCosLongitude) {
                *o = cs;
                o += pitch;
            }
            if (mask & kSinLongitude) *o = sn;
        }
    }
}

enum : uint32_t { kAzimuth = 1u << 0, kZenith = 1u << 1 };

__global__ void __launch_bounds__(kBlock)
obs_view_angles_kernel(const double* __restrict__ latitude, const double* __restrict__ longitude, const double* __restrict__ sat_latitude,
                       const double* __restrict__ sat_longitude, int64_t n, uint32_t flags, double* __restrict__ out, int64_t pitch) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const double latdeg = latitude[i], londeg = longitude[i], satlat = sat_latitude[i], satlon = sat_longitude[i];
        const double lat = latdeg * kRad, lon = londeg * kRad, latS = satlat * kRad, lonS = satlon * kRad;
        double sin_lat, cos_lat, sin_latS, cos_latS, sin_dlon, cos_dlon;
        row_sincos(lat, sin_lat, cos_lat);
        row_sincos(latS, sin_latS, cos_latS);
        row_sincos(lon - lonS, sin_dlon, cos_dlon);  // sin for the azimuth (:73), cos for the zenith (:34): the same difference
        double* __restrict__ o = out + i;
        if (flags & kAzimuth) {
            // R: sat_view_angles.py:52-97
            double azimuth = 0.0;
            if (fabs(latdeg - satlat) > 0.00001 && fabs(londeg - satlon) > 0.00001) {
                const double zdlon = lonS - lon;
                const double zdlat = latS - lat;
                double s_half_lat, s_half_lon, unused;
                row_sincos(zdlat / 2.0, s_half_lat, unused);
                row_sincos(zdlon / 2.0, s_half_lon, unused);
                const double za = s_half_lat * s_half_lat + cos_lat * cos_latS * (s_half_lon * s_half_lon);
                const double root = sqrt(za);
                const double distOS = 2.0 * asin((root < 1.0 || root != root) ? root : 1.0);  // np.minimum(1.0, .): a NaN stays
                double sin_d, cos_d;
                row_sincos(distOS, sin_d, cos_d);
                double azmsin = cos_latS / sin_d * sin_dlon;
                azmsin = asin(numpy_clip(azmsin, -1.0, 1.0));
                double azmcos = (sin_latS - sin_lat * cos_d) / (cos_lat * sin_d);
                azmcos = acos(numpy_clip(azmcos, -1.0, 1.0));
                azmcos = azmsin > 0 ? -azmcos : azmcos;
                double azm = azmcos;
                azm = azm >= kPi ? azm - 2.0 * kPi : azm;
                azm = azm < -kPi ? azm + 2.0 * kPi : azm;
                azimuth = numpy_mod(azm * kDeg, 360.0);
            }
            *o = azimuth;
            o += pitch;
        }
        if (flags & kZenith) {
            // R: sat_view_angles.py:17-49 — a geostationary orbit
            const double rearth = 6378.170;
            const double satalt = 6610839 * 1.0e-6 * rearth - rearth;
            const double ds = rearth * 2 * asin(sqrt((1 - sin_lat * sin_latS - cos_lat * cos_latS * cos_dlon) / 2));
            const double a = ds / rearth;
            double sin_a, cos_a;
            row_sincos(a, sin_a, cos_a);
            const double rl = rearth * sin_a;
            const double rm = rearth * cos_a;
            const double tb = rl / (rearth + satalt - rm);
            const double b = atan(tb);
            *o = (a + b) * kDeg;
        }
    }
}

__global__ void __launch_bounds__(kBlock)
obs_planck_bt_kernel(const double* __restrict__ radiance, int64_t n, int64_t in_pitch, const double* __restrict__ a, const double* __restrict__ b,
                     double* __restrict__ out, int64_t out_pitch) {
    const int ch = blockIdx.y;
    const double a_ch = a[ch], b_ch = b[ch];
    const double* __restrict__ row = radiance + (int64_t)ch * in_pitch;
    double* __restrict__ dst = out + (int64_t)ch * out_pitch;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        // R: radiance_to_brightness_temperature.py:111-113
        const double R = row[i] * 1e-2;
        const double floored = (R >= 1e-300 || R != R) ? R : 1e-300;  // np.maximum(R, 1e-300): a NaN stays
        dst[i] = b_ch / log1p(a_ch / floored);
    }
}

}  // namespace atx

using namespace atx;

extern "C" int atx_obs_forcings(const int64_t* date_ns, const double* latitude, const double* longitude, int64_t n, uint32_t mask, double* out,
                                int64_t pitch, void* stream) {
    ATX_REQUIRE(n >= 0, ATX_EINVAL, "atx_obs_forcings: %lld rows", (long long)n);
    ATX_REQUIRE(mask != 0 && (mask & ~kAllForcings) == 0, ATX_EINVAL, "atx_obs_forcings: the mask %#x names no forcing, or one beyond the nine",
                (unsigned)mask);
    ATX_REQUIRE(pitch >= n, ATX_ESHAPE, "atx_obs_forcings: pitch %lld below n", (long long)pitch);
    if (n == 0) return ATX_OK;
    const bool need_date = mask & (kCosJulianDay | kSinJulianDay | kCosSza | kSinLocalTime | kCosLocalTime);
    const bool need_lat = mask & (kCosSza | kCosLatitude | kSinLatitude);
    const bool need_lon = mask & (kCosSza | kSinLocalTime | kCosLocalTime | kCosLongitude | kSinLongitude);
    ATX_REQUIRE(out && (date_ns || !need_date) && (latitude || !need_lat) && (longitude || !need_lon), ATX_EINVAL,
                "atx_obs_forcings: null pointer");
    hipLaunchKernelGGL(obs_forcings_kernel, dim3(row_grid(n)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), date_ns, latitude, longitude, n,
                       mask, out, pitch);
    ATX_LAUNCH_CHECK("obs_forcings");
    return ATX_OK;
}

extern "C" int atx_obs_view_angles(const double* latitude, const double* longitude, const double* sat_latitude, const double* sat_longitude,
                                   int64_t n, uint32_t flags, double* out, int64_t pitch, void* stream) {
    ATX_REQUIRE(n >= 0, ATX_EINVAL, "atx_obs_view_angles: %lld rows", (long long)n);
    ATX_REQUIRE(flags != 0 && (flags & ~(kAzimuth | kZenith)) == 0, ATX_EINVAL, "atx_obs_view_angles: flags %#x (1: azimuth, 2: zenith)",
                (unsigned)flags);
    ATX_REQUIRE(pitch >= n, ATX_ESHAPE, "atx_obs_view_angles: pitch %lld below n", (long long)pitch);
    if (n == 0) return ATX_OK;
    ATX_REQUIRE(latitude && longitude && sat_latitude && sat_longitude && out, ATX_EINVAL, "atx_obs_view_angles: null pointer");
    hipLaunchKernelGGL(obs_view_angles_kernel, dim3(row_grid(n)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), latitude, longitude,
                       sat_latitude, sat_longitude, n, flags, out, pitch);
    ATX_LAUNCH_CHECK("obs_view_angles");
    return ATX_OK;
}

extern "C" int atx_obs_planck_bt(const double* radiance, int64_t n, int32_t n_ch, int64_t in_pitch, const double* a, const double* b, double* out,
                                 int64_t out_pitch, void* stream) {
    ATX_REQUIRE(n >= 0, ATX_EINVAL, "atx_obs_planck_bt: %lld rows", (long long)n);
    ATX_REQUIRE(n_ch > 0 && n_ch <= 65535, ATX_EINVAL, "atx_obs_planck_bt: 1 .. 65535 channels, got %d", (int)n_ch);
    ATX_REQUIRE(in_pitch >= n && out_pitch >= n, ATX_ESHAPE, "atx_obs_planck_bt: pitch %lld / %lld below n", (long long)in_pitch,
                (long long)out_pitch);
    if (n == 0) return ATX_OK;
    ATX_REQUIRE(radiance && a && b && out, ATX_EINVAL, "atx_obs_planck_bt: null pointer");
    const unsigned gx = row_grid(n);
    hipLaunchKernelGGL(obs_planck_bt_kernel, dim3(gx, (unsigned)n_ch), dim3(kBlock), 0, static_cast<hipStream_t>(stream), radiance, n, in_pitch, a,
                       b, out, out_pitch);
    ATX_LAUNCH_CHECK("obs_planck_bt");
    return ATX_OK;
}
