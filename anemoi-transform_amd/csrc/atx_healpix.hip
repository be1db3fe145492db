// HEALPix pixel indices of (longitude, latitude) rows: atx_healpix_ang2pix.  float64 in, int64 out, one lane per row.
//
// The reference's add_healpix filter is one line, hp.ang2pix(nside, lon, lat, nest=True, lonlat=True) (R: filters/tabular/add_healpix.py:43-51);
// everything behind it is healpy's lonlat2thetaphi and healpix_cxx's ang2pix -> loc2pix.  The pixelisation is a closed-form statement
// (Gorski et al. 2005, ApJ 622, 759), restated here for both orderings: NESTED, which the filter asks for, and RING, which the reference's
// "h<nside>" grids are listed in (R: support/superob.py:28-40).  tests/healpix_restatement.py holds the same statement in numpy.
//
// Numerics.  theta, phi, tt, fmod, the products and the truncations are evaluated literal for literal in the operation
// order of the source, with IEEE division and without contraction (-ffp-contract=off), so they have numpy's bits.  cos / sin of theta
// are sincos_moderate (atx_common.hpp, < 1 ulp; a valid theta lies in [0, pi], far inside its range), sqrt is correctly rounded.  Away
// from a pixel edge the index is therefore the exact geometry's; ON an edge the last bit of cos / sin decides between the two
// neighbouring pixels, as it does between two builds of healpy.
//
// Launch shape, as atx_obs_rowops.hip: VALU-bound (one float64 sincos, an fmod and a sqrt per row against 24 bytes of traffic), one row
// per lane, 256-lane workgroups, a grid-stride loop under a grid cap; a wave reads two contiguous 512-byte runs and writes one.  The
// scheme and the order are uniform over the launch (scalar branches); the region branch — equatorial belt or polar cap — diverges by
// nature.  A row that has no pixel (NaN or out-of-range latitude, non-finite longitude) gets -1 and is counted, one atomic per wave as
// atx_check_indices counts; such a row's doubles are never converted to integers.
#include "atx_common.hpp"

namespace atx {

constexpr double kHpPi = 3.141592653589793;     // np.pi
constexpr double kHpRad = kHpPi / 180.0;        // np.radians: x * (pi / 180)
constexpr double kHpHalfPi = kHpPi / 2.0;       // np.pi / 2.0
constexpr double kHpInvHalfPi = 2.0 / kHpPi;    // healpix_cxx's inv_halfpi
constexpr double kHpTwoThird = 2.0 / 3.0;       // healpix_cxx's twothird
constexpr int kHpGrid = 1 << 20;                // grid cap: 2^28 rows before a lane takes a second one
constexpr int64_t kHpMaxNside = 1ll << 29;      // healpix_cxx's order_max for 64-bit indices

// healpix_cxx's fmodulo(v, 4.0): v modulo 4 in [0, 4).
__device__ __forceinline__ double fmodulo4(double v) {
    if (v >= 0.0) return v < 4.0 ? v : fmod(v, 4.0);
    const double t = fmod(v, 4.0) + 4.0;
    return t == 4.0 ? 0.0 : t;  // a tiny negative v rounds up to 4
}

// Bit b of x (x < 2^32) to bit 2b: the 64-bit mask-and-shift ladder.
__device__ __forceinline__ uint64_t spread_bits(uint64_t x) {
    x = (x | (x << 16)) & 0x0000ffff0000ffffull;
    x = (x | (x << 8)) & 0x00ff00ff00ff00ffull;
    x = (x | (x << 4)) & 0x0f0f0f0f0f0f0f0full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return x;
}

__global__ void __launch_bounds__(kBlock)
healpix_ang2pix_kernel(const double* __restrict__ longitude, const double* __restrict__ latitude, int64_t n, int64_t nside, int order, int nest,
                       int64_t* __restrict__ pix, unsigned long long* n_bad) {
    const double dnside = (double)nside;  // exact: nside <= 2^29
    const int64_t nl4 = 4 * nside;
    const int64_t ncap = 2 * nside * (nside - 1);
    const int64_t npix = 12 * nside * nside;
    unsigned long long bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const double lon = longitude[i], lat = latitude[i];
        // healpy lonlat2thetaphi
        const double theta = kHpHalfPi - lat * kHpRad;
        const double phi = lon * kHpRad;
        // healpy's check_theta_valid; a NaN latitude fails the first comparison, fabs(lon) < inf is false for NaN and +-inf
        if (!(theta >= 0.0 && theta <= kHpPi) || !(fabs(lon) < __builtin_huge_val())) {
            pix[i] = -1;
            bad += 1;
            continue;
        }
        // healpix_cxx ang2pix -> loc2pix
        double sth, z;
        sincos_moderate(theta, sth, z);  // theta in [0, pi]: always served
        const bool have_sth = theta < 0.01 || theta > 3.14159 - 0.01;
        const double za = fabs(z);
        const double tt = fmodulo4(phi * kHpInvHalfPi);  // in [0, 4)
        int64_t result;
        if (za <= kHpTwoThird) {  // equatorial region
            const double t1 = dnside * (0.5 + tt);
            const double t2 = dnside * (z * 0.75);
            const int64_t jp = (int64_t)(t1 - t2);  // index of ascending edge line, in [0, 5 nside)
            const int64_t jm = (int64_t)(t1 + t2);  // index of descending edge line, in [0, 5 nside)
            if (nest) {
                const int64_t ifp = jp >> order;  // in {0 .. 4}
                const int64_t ifm = jm >> order;
                const int64_t face = (ifp == ifm) ? (ifp | 4) : ((ifp < ifm) ? ifp : (ifm + 8));
                const int64_t ix = jm & (nside - 1);
                const int64_t iy = nside - (jp & (nside - 1)) - 1;
                result = face * nside * nside + (int64_t)(spread_bits((uint64_t)ix) + 2 * spread_bits((uint64_t)iy));
            } else {
                const int64_t ir = nside + 1 + jp - jm;  // ring number counted from z = 2/3, in {1 .. 2 nside + 1}
                const int64_t kshift = 1 - (ir & 1);     // 1 if ir is even
                // (...) >> 1 lies in [4 nside - 1, 8 nside]: mod 4 nside is at most two subtractions, for any nside
                int64_t ip = (jp + jm - nside + kshift + 1 + nl4 + nl4) >> 1;
                while (ip >= nl4) ip -= nl4;
                result = ncap + (ir - 1) * nl4 + ip;
            }
        } else {  // polar caps
            const int64_t ntt = (int64_t)tt < 3 ? (int64_t)tt : 3;
            const double tp = tt - (double)ntt;
            const double tmp = (za < 0.99 || !have_sth) ? dnside * sqrt(3 * (1 - za)) : dnside * sth / sqrt((1. + za) / 3.);
            int64_t jp = (int64_t)(tp * tmp);          // increasing edge line index
            int64_t jm = (int64_t)((1.0 - tp) * tmp);  // decreasing edge line index
            if (nest) {
                jp = jp < nside - 1 ? jp : nside - 1;  // for points too close to the boundary
                jm = jm < nside - 1 ? jm : nside - 1;
                const int64_t ix = z >= 0 ? nside - jm - 1 : jp;
                const int64_t iy = z >= 0 ? nside - jp - 1 : jm;
                const int64_t face = z >= 0 ? ntt : ntt + 8;
                result = face * nside * nside + (int64_t)(spread_bits((uint64_t)ix) + 2 * spread_bits((uint64_t)iy));
            } else {
                const int64_t ir = jp + jm + 1;                  // ring number counted from the closest pole
                const int64_t ip = (int64_t)(tt * (double)ir);  // in {0 .. 4 ir - 1}
                result = z > 0 ? 2 * ir * (ir - 1) + ip : npix - 2 * ir * (ir + 1) + ip;
            }
        }
        pix[i] = result;
    }
    // wavefront (64-lane) shuffle reduction, then one atomic per wave
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) bad += __shfl_down(bad, off, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0 && bad) atomicAdd(n_bad, bad);
}

}  // namespace atx

using namespace atx;

extern "C" int atx_healpix_ang2pix(const double* longitude, const double* latitude, int64_t n, int64_t nside, int scheme, int64_t* pix,
                                   int64_t* n_bad, void* stream) {
    ATX_REQUIRE(n >= 0, ATX_EINVAL, "atx_healpix_ang2pix: %lld rows", (long long)n);
    ATX_REQUIRE(nside >= 1 && nside <= kHpMaxNside, ATX_EINVAL, "atx_healpix_ang2pix: nside %lld outside 1 .. 2^29", (long long)nside);
    ATX_REQUIRE(scheme == ATX_HEALPIX_RING || scheme == ATX_HEALPIX_NEST, ATX_EINVAL, "atx_healpix_ang2pix: scheme %d (0: ring, 1: nest)", scheme);
    ATX_REQUIRE(scheme == ATX_HEALPIX_RING || (nside & (nside - 1)) == 0, ATX_EINVAL,
                "atx_healpix_ang2pix: the nested scheme needs an nside that is a power of two, got %lld", (long long)nside);
    if (n == 0) return ATX_OK;
    ATX_REQUIRE(longitude && latitude && pix && n_bad, ATX_EINVAL, "atx_healpix_ang2pix: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int st = hip_status(hipMemsetAsync(n_bad, 0, sizeof(int64_t), s), "atx_healpix_ang2pix memset");
    if (st != ATX_OK) return st;
    int order = 0;  // log2(nside), used by the nested scheme only
    while ((int64_t(1) << order) < nside) ++order;
    hipLaunchKernelGGL(healpix_ang2pix_kernel, dim3(grid_for(n, kBlock, kHpGrid)), dim3(kBlock), 0, s, longitude, latitude, n,
                       nside, order, scheme == ATX_HEALPIX_NEST ? 1 : 0, pix, reinterpret_cast<unsigned long long*>(n_bad));
    ATX_LAUNCH_CHECK("healpix_ang2pix");
    return ATX_OK;
}
