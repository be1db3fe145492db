// log and exp for the parcel ascent, within 0.54 and 0.61 ulp of the true value (glibc: 0.52 and 0.51) (measured on the host against 80-bit arithmetic,
// 4 M arguments each over the ranges the kernels pass: pressures, temperatures, ratios near 1; exponents in [-12, 4]).
//
// The statement's areas multiply b by ln p_lower - ln p_upper: two logarithms near 11.5 whose difference is 0.02 .. 0.2, so one ulp of a
// logarithm is tens of ulps of an area, and the Newton residual divides the rounding of log T by F' ~ 1 / T.  atx_log and atx_exp are
// budgeted at 1 ulp (true errors 0.73 and 0.9): enough for the operators they were written for, twice glibc's here.  These two keep the
// leading term of the result in two words until the last addition, so that addition's rounding is nearly all the error there is:
//   log   x = 2^k m, m in [sqrt(1/2), sqrt(2)), f = m - 1 (exact), s = f / (2 + f) as s_hi + s_lo (the residual by fma),
//         log m = 2 s_hi + (2 s_lo + s_hi z R(z)), z = s_hi^2, R the series 2/3 + 2 z/5 + ... to z^11 (|s| <= 0.1716: the first term left
//         out is below 2^-63 of the result); k ln2 in two words, the first with 42 bits so that k ln2_hi is exact;
//   exp   x = k ln2 + r, r = r_hi + r_lo with r_hi EXACT (ln2_hi has 42 bits, |x| >= 0.34 is a multiple of 2^-54),
//         e^r = (1 + r_hi) + (r_hi^2 P(r_hi) + r_lo e^r_hi), 1 + r_hi as a two-sum, P the series 1/2 + r/6 + ... to r^12.
// Positive normal finite arguments of log and |x| < 700 of exp only; everything else goes to atx_log / atx_exp, which follow IEEE.
#pragma once

#ifndef ATX_PARCEL_HD
#define ATX_PARCEL_HD __host__ __device__ __forceinline__
#endif

namespace atx {

// x = m 2^k with m in [0.5, 1), and m 2^k back
ATX_PARCEL_HD double parcel_frexp(double x, int& k) {
#if defined(__HIP_DEVICE_COMPILE__)
    k = __builtin_amdgcn_frexp_exp(x);
    return __builtin_amdgcn_frexp_mant(x);
#else
    return __builtin_frexp(x, &k);
#endif
}
ATX_PARCEL_HD double parcel_ldexp(double m, int k) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_ldexp(m, k);
#else
    return __builtin_ldexp(m, k);
#endif
}

// log of a positive, normal, finite x
ATX_PARCEL_HD double parcel_log_normal(double x) {
    constexpr double ln2_hi = 0x1.62e42fefa38p-1, ln2_lo = 0x1.ef35793c7673p-45;  // 42 bits, and ln 2 - ln2_hi
    int k;
    double m = parcel_frexp(x, k);
    if (m < 0.70710678118654752440) m = m * 2.0, k -= 1;
    const double f = m - 1.0;  // exact
    const double den = 2.0 + f, den_lo = (2.0 - den) + f;  // (Fast2Sum: |f| < 2)
    const double s = f / den;
    const double s_lo = (__builtin_fma(-s, den, f) - s * den_lo) / den;
    const double z = s * s;
    double R = 2.0 / 23.0;
    R = __builtin_fma(R, z, 2.0 / 21.0);
    R = __builtin_fma(R, z, 2.0 / 19.0);
    R = __builtin_fma(R, z, 2.0 / 17.0);
    R = __builtin_fma(R, z, 2.0 / 15.0);
    R = __builtin_fma(R, z, 2.0 / 13.0);
    R = __builtin_fma(R, z, 2.0 / 11.0);
    R = __builtin_fma(R, z, 2.0 / 9.0);
    R = __builtin_fma(R, z, 2.0 / 7.0);
    R = __builtin_fma(R, z, 2.0 / 5.0);
    R = __builtin_fma(R, z, 2.0 / 3.0);
    const double dk = (double)k;
    const double tail = __builtin_fma(s * z, R, 2.0 * s_lo);
    const double a = dk * ln2_hi, b = 2.0 * s;  // a is exact; |a| >= |b| or a == 0
    const double hi = a + b, err = (a - hi) + b;
    return hi + (err + __builtin_fma(dk, ln2_lo, tail));
}

// exp of |x| < 700
ATX_PARCEL_HD double parcel_exp_moderate(double x) {
    constexpr double log2e = 1.4426950408889634, ln2_hi = 0x1.62e42fefa38p-1, ln2_lo = 0x1.ef35793c7673p-45;
    const double k = __builtin_rint(x * log2e);
    const double r = __builtin_fma(-k, ln2_hi, x);  // exact
    const double r_lo = -k * ln2_lo;
    double P = 1.0 / 87178291200.0;  // 1 / 14!
    P = __builtin_fma(P, r, 1.0 / 6227020800.0);
    P = __builtin_fma(P, r, 1.0 / 479001600.0);
    P = __builtin_fma(P, r, 1.0 / 39916800.0);
    P = __builtin_fma(P, r, 1.0 / 3628800.0);
    P = __builtin_fma(P, r, 1.0 / 362880.0);
    P = __builtin_fma(P, r, 1.0 / 40320.0);
    P = __builtin_fma(P, r, 1.0 / 5040.0);
    P = __builtin_fma(P, r, 1.0 / 720.0);
    P = __builtin_fma(P, r, 1.0 / 120.0);
    P = __builtin_fma(P, r, 1.0 / 24.0);
    P = __builtin_fma(P, r, 1.0 / 6.0);
    P = __builtin_fma(P, r, 0.5);
    const double hi = 1.0 + r, err = (1.0 - hi) + r;  // (Fast2Sum: |r| < 1)
    const double tail = __builtin_fma(r * r, P, err);
    return parcel_ldexp(hi + __builtin_fma(r_lo, hi + tail, tail), (int)k);  // (r_lo e^r: the factor needs no more than its first rounding)
}

}  // namespace atx
