// Temperature and geopotential on pressure levels with the IFS extrapolations under the ground, and mean sea level pressure:
// atx_pltz_interpolate (include/atx_pltz.h holds the statement), built into a library of its own, lib/libatx_pltz.so — the entry points
// and the kernels of libatx_levels, libatx_geopotential and libatx_heights are fixed, tested sets, as libatx's are.  The hydrostatic sum
// of atx_geopotential.hip, the bracket search of atx_levels.hip, the interpolation of t and of c, the extrapolations and msl are ONE
// launch here, and c is never written to HBM.  The terms and the sum are a copy of atx_heights.hip's statements: the libraries share no
// code beyond the headers under csrc/.
//
// ATX_COLUMNS, a 256-lane workgroup per tile of PT consecutive points (atx_column_tile.hpp), the phases in order:
//   1. stage     the tile's t columns and its q columns into LDS (stage_columns, the route decided per stack); A and B of the
//                n_lev + 1 half levels the rows touch; one lane per point: sp and zs, float64;
//   2. terms     one lane per (point, level): (alpha r) t and (delta r) t into LDS — the logarithm and the two divisions, 256 lanes
//                wide — and whether the point's p_full ever decreases.  Unlike the heights kernel's, t outlives the integral: it is
//                interpolated afterwards.  So the alpha terms get a float64 array of their own (odd pitch) in both widths; the delta
//                terms of a float64 stack take q's place, a float32 stack's an array of their own;
//   3. sum       one lane per point, from the ground up: the sequential chain of adds with kPltzBatch LDS reads in flight ahead of it.
//                Meanwhile the lanes at the OTHER end of the workgroup, another wave, take one point each: T*, T0, aZ, Tz into LDS and
//                msl (the one exponential of a point) into the point's output row in LDS;
//                then, one lane per (point, level) again, c[k] = zs + (S[k] + a[k]) into the place of a[k];
//   4. targets   one lane per (point, target): the count over the point's p_full, which is RECOMPUTED from the staged coefficients and
//                sp — where it never decreases the count is what a bisection finds, 8 steps of two multiply-adds for 137 levels,
//                cheaper than 1 KiB of LDS per point, which would cost a tile a quarter of its points; any other column is counted
//                level by level — then BOTH outputs of the pair into the point's output row in LDS; log(P / p_g) only under the ground;
//   5. store     one lane per output element, in output order: a point's 2 n_tgt (+ 1) values are one contiguous run in HBM.
// LDS per (point, level): 24 bytes in either width; 137 levels and 13 targets leave 9 points to a tile of 32 KiB.  ATX_FIELDS: one lane
// per point, the plain reading of the statement: per target the count, then the column from the ground up as far as level a for c[a]
// and c[b].  Both layouts and every load route evaluate the same float64 statements in the same order (target_values, point_terms,
// msl_value serve both): same bits.  No scratch (profiles/pltz_resources.json).
#include "../../../include/atx_pltz.h"
#include "../atx_column_tile.hpp"

namespace atx {

constexpr int kPltzMaxLevels = ATX_PLTZ_MAX_LEVELS;
constexpr int kPltzBatch = 8;                            // LDS reads of the sum phase in flight ahead of the dependent adds
constexpr double kPltzRd = 287.0597, kPltzRv = 461.5250;  // J / (kg K), as in atx_geopotential.hip
constexpr double kPltzLn2 = 0.6931471805599453;          // alpha of the IFS top level
constexpr double kPltzG = 9.80665, kPltzGamma = 0.0065;  // m / s^2;  K / m, the standard lapse rate
constexpr double kPltzKappa = kPltzGamma * kPltzRd / kPltzG;

// The two terms of one (point, level), the statement of include/atx_geopotential.h: `a` = (alpha r) t, `d` = (delta r) t (0.0 and unused at j == 0).
struct PltzTerms {
    double a, d;
};
__device__ __forceinline__ PltzTerms pltz_terms(int j, double p_up, double p_dn, double t, double q) {
    const double om = 1.0 - q;
    const double dry = kPltzRd * om, wet = kPltzRv * q;
    const double r = dry + wet;
    PltzTerms g;
    if (j == 0) {
        g.a = (kPltzLn2 * r) * t;
        g.d = 0.0;
        return g;
    }
    const double ratio = p_dn / p_up;  // IEEE division
    const double delta = atx_log(ratio);
    const double thick = p_dn - p_up;
    const double w = p_up / thick;  // IEEE division
    const double wd = w * delta;
    const double alpha = 1.0 - wd;
    g.a = (alpha * r) * t;
    g.d = (delta * r) * t;
    return g;
}

// c[k] of the statement from the sum of the deltas below the level and the level's own alpha term.
__device__ __forceinline__ double pltz_level_geopotential(double zs, double below, double own) {
    const double lower = below + own;
    return zs + lower;
}

template <bool LOG>
__device__ __forceinline__ double pltz_coordinate(double p) {
    if constexpr (LOG) return atx_log(p);
    return p;
}

// What a point's extrapolations share: no library function in any of it.
struct PltzPoint {
    double tstar, t0, alpha, tz;
};
__device__ __forceinline__ PltzPoint point_terms(double t_low, double p_low, double p_ground, double zs) {
    PltzPoint r;
    const double hgt = zs / kPltzG;
    const double ratio = p_ground / p_low;
    const double excess = ratio - 1.0;
    const double slope = kPltzKappa * t_low;
    const double rise = slope * excess;
    r.tstar = t_low + rise;
    const double lapse = kPltzGamma * hgt;
    r.t0 = r.tstar + lapse;
    r.alpha = kPltzKappa;
    r.tz = r.tstar;
    if (r.tstar <= 290.5 && r.t0 > 290.5) {
        const double gap = 290.5 - r.tstar;
        const double scaled = kPltzRd * gap;
        r.alpha = scaled / zs;
    }
    if (r.tstar > 290.5 && r.t0 > 290.5) {
        r.alpha = 0.0;
        const double sum = 290.5 + r.tstar;
        r.tz = 0.5 * sum;
    }
    if (r.tz < 255.0) {
        const double sum = 255.0 + r.tz;
        r.tz = 0.5 * sum;
    }
    return r;
}

// msl of the statement (rule 6; rule 1 is the caller's).
__device__ __forceinline__ double msl_value(const PltzPoint& pt, double p_ground, double zs) {
    if (__builtin_fabs(zs) < 0.001) return p_ground;
    const double rt = kPltzRd * pt.tz;
    const double h = zs / rt;
    const double az = pt.alpha * zs;
    const double x = az / rt;
    const double half = x / 2.0;
    const double one = 1.0 - half;
    const double xx = x * x;
    const double third = xx / 3.0;
    const double series = one + third;
    const double arg = h * series;
    const double e = atx_exp(arg);
    return p_ground * e;
}

// One NaN for every way to it (a rule of the statement, or a NaN that t, q or the table brought along): the layouts agree in every byte.
template <typename T>
__device__ __forceinline__ T pltz_store(double y, bool nan) {
    return nan || y != y ? quiet_nan<T>() : (T)y;
}

struct PltzPair {
    double t, z;
    bool nan;
};

// Rules 1 to 5 of the statement after the count: `pf(k)`, `tt(k)` and `cc(k)` give p[k], t[k] and c[k] of the point.
template <bool LOG, typename PF, typename TT, typename CC>
__device__ __forceinline__ PltzPair target_values(int count, int n, double P, double sp, double zs, double p_ground, const PltzPoint& pt, PF&& pf,
                                                  TT&& tt, CC&& cc) {
    PltzPair r;
    r.t = r.z = 0.0;
    r.nan = true;
    if (sp != sp || zs != zs || count == 0) return r;
    if (count < n || P <= p_ground) {  // the interior, or the lowest half layer with (p_g, T*, zs) as its lower end
        const int a = count < n ? count - 1 : n - 1;
        const double p_b = count < n ? pf(count) : p_ground;
        const double tb = count < n ? tt(count) : pt.tstar, cb = count < n ? cc(count) : zs;
        const double ca = pltz_coordinate<LOG>(pf(a)), cbb = pltz_coordinate<LOG>(p_b), cp = pltz_coordinate<LOG>(P);
        const double w = (cp - ca) / (cbb - ca);  // IEEE division
        const double ta = tt(a), za = cc(a);
        const double dt = tb - ta, dz = cb - za;
        const double st = w * dt, sz = w * dz;
        r.t = ta + st;
        r.z = za + sz;
        r.nan = false;
        return r;
    }
    if (!(P > p_ground)) return r;
    const double ratio = P / p_ground;  // IEEE division
    const double l = atx_log(ratio);
    const double hgt = zs / kPltzG;
    double y;
    if (hgt < 2000.0) {
        y = kPltzKappa * l;
    } else {
        const double plateau = pt.t0 < 298.0 ? pt.t0 : 298.0;
        double t0p = plateau;
        if (!(hgt > 2500.0)) {
            const double wa = 2500.0 - hgt, wb = hgt - 2000.0;
            const double pa = wa * pt.t0, pb = wb * plateau;
            const double mix = pa + pb;
            t0p = 0.002 * mix;
        }
        if (t0p < pt.tstar) {
            y = 0.0;
        } else {
            const double gap = t0p - pt.tstar;
            const double scaled = kPltzRd * gap;
            const double rate = scaled / zs;
            y = rate * l;
        }
    }
    {
        const double y2 = y * y;
        const double y3 = y2 * y;
        const double s1 = 1.0 + y;
        const double h2 = y2 / 2.0;
        const double s2 = s1 + h2;
        const double h3 = y3 / 6.0;
        const double s3 = s2 + h3;
        r.t = pt.tstar * s3;
    }
    {
        const double yz = pt.alpha * l;
        const double rt = kPltzRd * pt.tz;
        const double lead = rt * l;
        const double half = yz / 2.0;
        const double s1 = 1.0 + half;
        const double sq = yz * yz;
        const double sixth = sq / 6.0;
        const double s2 = s1 + sixth;
        const double drop = lead * s2;
        r.z = zs - drop;
    }
    r.nan = false;
    return r;
}

// Where the LDS of a tile of `pt` points holds what (byte offsets, multiples of 16): one definition for the launch and the kernel.
// `ta` holds the alpha terms, then c; `td` the delta terms, then their sums from the ground — a float64 stack's in q's place.
struct PltzCarve {
    int64_t t, q, td, ta, sps, zss, tstar, t0, alpha, tz, outs, mono, coef, total;
    int pa, pd;  // elements between two points' terms
};
__host__ __device__ inline PltzCarve pltz_carve(int64_t pt, int lt, int lq, int elem, int n_lev, int rows) {
    PltzCarve c;
    c.pa = n_lev | 1;                              // odd: the points of the sum phase fall into different banks
    c.t = 0;                                       // T [pt][lt]
    c.q = round16(pt * lt * elem);                 // T [pt][lq]
    int64_t end = c.q + round16(pt * lq * elem);
    if (elem == 8) {
        c.td = c.q, c.pd = lq;
    } else {
        c.td = end, c.pd = c.pa;                   // double [pt][pd]
        end = c.td + round16(pt * c.pd * 8);
    }
    c.ta = end;                                    // double [pt][pa]
    c.sps = c.ta + round16(pt * c.pa * 8);         // double [pt], and so are the five that follow
    c.zss = c.sps + round16(pt * 8);
    c.tstar = c.zss + round16(pt * 8);
    c.t0 = c.tstar + round16(pt * 8);
    c.alpha = c.t0 + round16(pt * 8);
    c.tz = c.alpha + round16(pt * 8);
    c.outs = c.tz + round16(pt * 8);               // T [pt][rows]
    c.mono = c.outs + round16(pt * rows * elem);   // int [pt]
    c.coef = c.mono + round16(pt * 4);             // double [2][n_lev + 1]
    c.total = c.coef + round16((int64_t)2 * (n_lev + 1) * 8);
    return c;
}

// ---- ATX_COLUMNS ---------------------------------------------------------------------------------------------------------------------
// VT, VQ: elements per load of the staging of t and of q (Vec16<T>::N, or 1 for an odd pitch or an unaligned base); lt, lq: elements
// between the columns of two points in LDS; rows: 2 n_tgt, or 2 n_tgt + 1 with msl.
template <typename T, int VT, int VQ, bool LOG>
__global__ void __launch_bounds__(kTileBlock)
pltz_columns_kernel(const T* __restrict__ t, const T* __restrict__ q, const T* __restrict__ sp, const T* __restrict__ zs, T* __restrict__ out,
                    const double* __restrict__ A, const double* __restrict__ B, const double* __restrict__ targets, int64_t n_pts, int n_lev, int n_tgt,
                    int first, int64_t t_pitch, int64_t q_pitch, int64_t out_pitch, int PT, int lt, int lq, int rows) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const PltzCarve lds = pltz_carve(PT, lt, lq, (int)sizeof(T), n_lev, rows);
    T* ts = reinterpret_cast<T*>(smem + lds.t);
    T* qs = reinterpret_cast<T*>(smem + lds.q);
    double* ta = reinterpret_cast<double*>(smem + lds.ta);  // the alpha terms, then c
    double* td = reinterpret_cast<double*>(smem + lds.td);
    double* sps = reinterpret_cast<double*>(smem + lds.sps);
    double* zss = reinterpret_cast<double*>(smem + lds.zss);
    double* tstars = reinterpret_cast<double*>(smem + lds.tstar);
    double* t0s = reinterpret_cast<double*>(smem + lds.t0);
    double* alphas = reinterpret_cast<double*>(smem + lds.alpha);
    double* tzs = reinterpret_cast<double*>(smem + lds.tz);
    T* outs = reinterpret_cast<T*>(smem + lds.outs);
    int* mono = reinterpret_cast<int*>(smem + lds.mono);  // 1: the point's p_full never decreases (and so holds no NaN)
    double* cA = reinterpret_cast<double*>(smem + lds.coef);  // A[first + k], k = 0 .. n_lev
    double* cB = cA + (n_lev + 1);
    const int pa = lds.pa, pd = lds.pd;

    const int tid = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * PT;
    const int npt = (int)(n_pts - p0 < PT ? n_pts - p0 : PT);

    // 1. stage
    stage_columns<T, VT>(t, ts, p0, npt, t_pitch, lt, tid);
    stage_columns<T, VQ>(q, qs, p0, npt, q_pitch, lq, tid);
    for (int k = tid; k <= n_lev; k += kTileBlock) {
        cA[k] = A[first + k];
        cB[k] = B[first + k];
    }
    for (int pt = tid; pt < npt; pt += kTileBlock) {
        sps[pt] = (double)sp[p0 + pt];
        zss[pt] = (double)zs[p0 + pt];
        mono[pt] = 1;
    }
    __syncthreads();
    // 2. terms
    TileWalk terms(tid, n_lev);
    for (int i = tid; i < npt * n_lev; i += kTileBlock, terms.next()) {
        const int pt = terms.row, k = terms.col;
        const double s = sps[pt];
        const double p_up = half_level(cA, cB, k, s), p_dn = half_level(cA, cB, k + 1, s);
        const double tk = (double)ts[pt * lt + k], qk = (double)qs[pt * lq + k];
        const PltzTerms g = pltz_terms(first + k, p_up, p_dn, tk, qk);
        ta[pt * pa + k] = g.a;
        td[pt * pd + k] = g.d;  // (float64: the place of qk, which only this lane reads)
        if (k + 1 < n_lev) {
            const double here = (p_up + p_dn) / 2.0, below = (p_dn + half_level(cA, cB, k + 2, s)) / 2.0;  // full_level's statements
            if (!(here <= below)) mono[pt] = 0;  // (a NaN fails too; every lane that writes, writes 0)
        }
    }
    __syncthreads();
    // 3. sum: S[k], the sum of d over the levels below k, replaces d[k] ...
    for (int pt = tid; pt < npt; pt += kTileBlock) {
        double* d = td + pt * pd;
        double S = 0.0;
        int k = n_lev - 1;
        for (; k >= kPltzBatch - 1; k -= kPltzBatch) {  // a batch of reads, then the dependent adds, then the writes
            double v[kPltzBatch];
#pragma unroll
            for (int i = 0; i < kPltzBatch; ++i) v[i] = d[k - i];
#pragma unroll
            for (int i = 0; i < kPltzBatch; ++i) {
                const double below = S;
                S = S + v[i];
                v[i] = below;
            }
#pragma unroll
            for (int i = 0; i < kPltzBatch; ++i) d[k - i] = v[i];
        }
        for (; k >= 0; --k) {
            const double below = S;
            S = S + d[k];  // (j == 0 adds 0.0 to a sum nothing reads again)
            d[k] = below;
        }
    }
    // ... while the lanes of the last wave take a point each: T*, T0, aZ, Tz, and msl
    for (int pt = kTileBlock - 1 - tid; pt < npt; pt += kTileBlock) {
        const double s = sps[pt], z0 = zss[pt];
        const double p_ground = half_level(cA, cB, n_lev, s), p_low = full_level(cA, cB, n_lev - 1, s);
        const PltzPoint r = point_terms((double)ts[pt * lt + n_lev - 1], p_low, p_ground, z0);
        tstars[pt] = r.tstar;
        t0s[pt] = r.t0;
        alphas[pt] = r.alpha;
        tzs[pt] = r.tz;
        if (rows > 2 * n_tgt) outs[pt * rows + 2 * n_tgt] = pltz_store<T>(msl_value(r, p_ground, z0), s != s || z0 != z0);
    }
    __syncthreads();
    // ... c[k] replaces a[k]
    TileWalk level(tid, n_lev);
    for (int i = tid; i < npt * n_lev; i += kTileBlock, level.next()) {
        const int pt = level.row, k = level.col;
        ta[pt * pa + k] = pltz_level_geopotential(zss[pt], td[pt * pd + k], ta[pt * pa + k]);
    }
    __syncthreads();
    // 4. targets
    if (n_tgt > 0) {
        TileWalk pair(tid, n_tgt);
        for (int i = tid; i < npt * n_tgt; i += kTileBlock, pair.next()) {
            const int pt = pair.row, tg = pair.col;
            const double P = targets[tg];
            const double s = sps[pt];
            auto pf = [&](int k) { return full_level(cA, cB, k, s); };
            int count = 0;
            if (mono[pt]) {  // #{k : p[k] <= P} of a column that never decreases: the first k with p[k] > P (a NaN target: 0)
                int hi = n_lev;
                while (count < hi) {
                    const int mid = (count + hi) >> 1;
                    if (pf(mid) <= P)
                        count = mid + 1;
                    else
                        hi = mid;
                }
            } else {
                for (int k = 0; k < n_lev; ++k) count += pf(k) <= P ? 1 : 0;
            }
            PltzPoint r;
            r.tstar = tstars[pt], r.t0 = t0s[pt], r.alpha = alphas[pt], r.tz = tzs[pt];
            const T* tcol = ts + pt * lt;
            const double* ccol = ta + pt * pa;
            const PltzPair y = target_values<LOG>(count, n_lev, P, s, zss[pt], half_level(cA, cB, n_lev, s), r, pf,
                                                  [&](int k) { return (double)tcol[k]; }, [&](int k) { return ccol[k]; });
            outs[pt * rows + tg] = pltz_store<T>(y.t, y.nan);
            outs[pt * rows + n_tgt + tg] = pltz_store<T>(y.z, y.nan);
        }
        __syncthreads();
    }
    // 5. store
    TileWalk store(tid, rows);
    for (int i = tid; i < npt * rows; i += kTileBlock, store.next()) out[(p0 + store.row) * out_pitch + store.col] = outs[i];
}

// ---- ATX_FIELDS ----------------------------------------------------------------------------------------------------------------------
template <typename T, bool LOG>
__global__ void __launch_bounds__(kTileBlock)
pltz_fields_kernel(const T* __restrict__ t, const T* __restrict__ q, const T* __restrict__ sp, const T* __restrict__ zs, T* __restrict__ out,
                   const double* __restrict__ A, const double* __restrict__ B, const double* __restrict__ targets, int64_t n_pts, int n_lev, int n_tgt,
                   int first, int64_t t_pitch, int64_t q_pitch, int64_t out_pitch, int rows) {
    const int64_t p = (int64_t)blockIdx.x * kTileBlock + threadIdx.x;
    if (p >= n_pts) return;
    const double s = (double)sp[p], z0 = (double)zs[p];
    const int L = n_lev - 1;
    const double p_ground = half_level(A, B, first + n_lev, s);
    auto pf = [&](int k) { return full_level(A, B, first + k, s); };  // (k is uniform: scalar loads of A, B)
    auto tt = [&](int k) { return (double)t[(int64_t)k * t_pitch + p]; };
    const PltzPoint r = point_terms(tt(L), pf(L), p_ground, z0);
    if (rows > 2 * n_tgt) out[(int64_t)2 * n_tgt * out_pitch + p] = pltz_store<T>(msl_value(r, p_ground, z0), s != s || z0 != z0);
    for (int tg = 0; tg < n_tgt; ++tg) {
        const double P = targets[tg];
        int count = 0;
        for (int k = 0; k < n_lev; ++k) count += pf(k) <= P ? 1 : 0;
        // the column from the ground up as far as level a, for c[a] and c[b] (c[b] alone in the lowest half layer)
        const int a = count < n_lev ? count - 1 : L;
        double ca = 0.0, cb = 0.0, S = 0.0;
        const bool walk = count > 0 && (count < n_lev || P <= p_ground) && s == s && z0 == z0;
        for (int k = L; walk && k >= a; --k) {
            const int j = first + k;
            const PltzTerms g = pltz_terms(j, half_level(A, B, j, s), half_level(A, B, j + 1, s), tt(k), (double)q[(int64_t)k * q_pitch + p]);
            cb = ca;
            ca = pltz_level_geopotential(z0, S, g.a);
            S = S + g.d;
        }
        const PltzPair y = target_values<LOG>(count, n_lev, P, s, z0, p_ground, r, pf, tt, [&](int k) { return k == a ? ca : cb; });
        out[(int64_t)tg * out_pitch + p] = pltz_store<T>(y.t, y.nan);
        out[(int64_t)(n_tgt + tg) * out_pitch + p] = pltz_store<T>(y.z, y.nan);
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
struct PltzCall {
    const void *t, *q, *sp, *zs;
    void* out;
    const double *A, *B, *targets;
    int64_t n_pts, t_pitch, q_pitch, out_pitch;
    int n_lev, n_tgt, first, layout, rows;
    bool log;
};

template <typename T>
static int pltz_typed(const PltzCall& c, hipStream_t st) {
    const char* fn = "atx_pltz_interpolate";
    const T* t = static_cast<const T*>(c.t);
    const T* q = static_cast<const T*>(c.q);
    const T* sp = static_cast<const T*>(c.sp);
    const T* zs = static_cast<const T*>(c.zs);
    T* out = static_cast<T*>(c.out);
    if (c.layout == ATX_FIELDS) {
        const dim3 grid((unsigned)((c.n_pts + kTileBlock - 1) / kTileBlock));
        with_flag(c.log, [&](auto flag) {
            hipLaunchKernelGGL((pltz_fields_kernel<T, decltype(flag)::value>), grid, dim3(kTileBlock), 0, st, t, q, sp, zs, out, c.A, c.B, c.targets, c.n_pts,
                               c.n_lev, c.n_tgt, c.first, c.t_pitch, c.q_pitch, c.out_pitch, c.rows);
            return 0;
        });
        ATX_LAUNCH_CHECK("pltz_fields");
        return ATX_OK;
    }
    constexpr int VEC = Vec16<T>::N;
    const ColumnRoute rt = column_route<VEC>(c.t, c.t_pitch, c.n_lev), rq = column_route<VEC>(c.q, c.q_pitch, c.n_lev);
    const int lt = rt.lds_pitch, lq = rq.lds_pitch;
    auto bytes = [&](int64_t pt) { return pltz_carve(pt, lt, lq, (int)sizeof(T), c.n_lev, c.rows).total; };
    const int PT = tile_points(bytes);
    ATX_REQUIRE(PT > 0, ATX_ENOTIMPL, "%s: one point's %d levels and %d output rows need %lld bytes of LDS, a workgroup has %lld", fn, c.n_lev, c.rows,
                (long long)bytes(1), (long long)kTileLdsLimit);
    const int64_t tiles = (c.n_pts + PT - 1) / PT;
    const size_t lds = (size_t)bytes(PT);
    with_flag(rt.vector, [&](auto vec_t) {
        return with_flag(rq.vector, [&](auto vec_q) {
            return with_flag(c.log, [&](auto flag) {
                constexpr int VT = decltype(vec_t)::value ? VEC : 1, VQ = decltype(vec_q)::value ? VEC : 1;
                hipLaunchKernelGGL((pltz_columns_kernel<T, VT, VQ, decltype(flag)::value>), dim3((unsigned)tiles), dim3(kTileBlock), lds, st, t, q, sp, zs, out,
                                   c.A, c.B, c.targets, c.n_pts, c.n_lev, c.n_tgt, c.first, c.t_pitch, c.q_pitch, c.out_pitch, PT, lt, lq, c.rows);
                return 0;
            });
        });
    });
    ATX_LAUNCH_CHECK("pltz_columns");
    return ATX_OK;
}

// The bytes [lo, hi) a stack of `rows` rows touches.
static void pltz_extent(const void* base, int64_t n_pts, int64_t rows, int64_t pitch, int layout, int elem, uintptr_t& lo, uintptr_t& hi) {
    const int64_t elements = layout == ATX_COLUMNS ? (n_pts - 1) * pitch + rows : (rows - 1) * pitch + n_pts;
    lo = reinterpret_cast<uintptr_t>(base);
    hi = lo + (uintptr_t)elements * (uintptr_t)elem;
}

}  // namespace atx

using namespace atx;

extern "C" int atx_pltz_version(void) { return ATX_PLTZ_VERSION; }

extern "C" const char* atx_pltz_last_error(void) { return last_error().c_str(); }

extern "C" int atx_pltz_interpolate(const void* t, const void* q, const void* sp, const void* zs, void* out, const double* A, const double* B,
                                    const double* targets, int64_t n_pts, int64_t n_lev, int64_t n_tgt, int64_t n_half, int64_t t_pitch, int64_t q_pitch,
                                    int64_t out_pitch, int dtype, int layout, int coordinate, int msl, void* stream) {
    const char* fn = "atx_pltz_interpolate";
    ATX_REQUIRE(dtype == ATX_F32 || dtype == ATX_F64, ATX_EINVAL, "%s: bad dtype %d", fn, dtype);
    ATX_REQUIRE(layout == ATX_COLUMNS || layout == ATX_FIELDS, ATX_EINVAL, "%s: bad layout %d", fn, layout);
    ATX_REQUIRE(coordinate == ATX_PLTZ_LINEAR || coordinate == ATX_PLTZ_LOG, ATX_EINVAL, "%s: unknown coordinate %d", fn, coordinate);
    ATX_REQUIRE(msl == 0 || msl == 1, ATX_EINVAL, "%s: msl=%d is neither 0 nor 1", fn, msl);
    ATX_REQUIRE(n_pts >= 0 && n_lev >= 1 && n_tgt >= 0, ATX_EINVAL, "%s: bad sizes n_pts=%lld n_lev=%lld n_tgt=%lld", fn, (long long)n_pts,
                (long long)n_lev, (long long)n_tgt);
    ATX_REQUIRE(n_half >= 2, ATX_EINVAL, "%s: n_half=%lld: a model has at least one level, two half levels", fn, (long long)n_half);
    ATX_REQUIRE(n_lev <= n_half - 1, ATX_EINVAL, "%s: n_lev=%lld rows are the lowest levels of a model of %lld, n_half=%lld", fn, (long long)n_lev,
                (long long)(n_half - 1), (long long)n_half);
    ATX_REQUIRE(n_lev <= kPltzMaxLevels, ATX_ENOTIMPL, "%s: n_lev=%lld exceeds the %d levels of one call", fn, (long long)n_lev, kPltzMaxLevels);
    ATX_REQUIRE(n_pts <= INT32_MAX && n_half <= 65535 && 2 * n_tgt + 1 <= 65535, ATX_ENOTIMPL,
                "%s: sizes exceed the indexing of one launch (n_pts=%lld n_lev=%lld n_tgt=%lld n_half=%lld)", fn, (long long)n_pts, (long long)n_lev,
                (long long)n_tgt, (long long)n_half);
    const int64_t rows = 2 * n_tgt + msl;
    if (layout == ATX_COLUMNS) {
        ATX_REQUIRE(t_pitch >= n_lev && q_pitch >= n_lev && out_pitch >= rows, ATX_ESHAPE, "%s: column pitch (%lld, %lld, %lld) < rows (%lld, %lld, %lld)", fn,
                    (long long)t_pitch, (long long)q_pitch, (long long)out_pitch, (long long)n_lev, (long long)n_lev, (long long)rows);
    } else {
        ATX_REQUIRE(t_pitch >= n_pts && q_pitch >= n_pts && out_pitch >= n_pts, ATX_ESHAPE, "%s: field pitch (%lld, %lld, %lld) < points %lld", fn,
                    (long long)t_pitch, (long long)q_pitch, (long long)out_pitch, (long long)n_pts);
    }
    ATX_REQUIRE(A && B, ATX_EINVAL, "%s: null A / B coefficients", fn);
    ATX_REQUIRE((t && q && sp && zs) || n_pts == 0, ATX_EINVAL, "%s: null t / q / sp / zs pointer", fn);
    ATX_REQUIRE(targets || n_tgt == 0, ATX_EINVAL, "%s: null targets", fn);
    ATX_REQUIRE(out || n_pts == 0 || rows == 0, ATX_EINVAL, "%s: null out pointer", fn);
    if (n_pts == 0 || rows == 0) return ATX_OK;
    const int elem = dtype == ATX_F32 ? 4 : 8;
    uintptr_t olo, ohi, lo, hi;
    pltz_extent(out, n_pts, rows, out_pitch, layout, elem, olo, ohi);
    pltz_extent(t, n_pts, n_lev, t_pitch, layout, elem, lo, hi);
    ATX_REQUIRE(!(olo < hi && lo < ohi), ATX_EINVAL, "%s: out overlaps t", fn);
    pltz_extent(q, n_pts, n_lev, q_pitch, layout, elem, lo, hi);
    ATX_REQUIRE(!(olo < hi && lo < ohi), ATX_EINVAL, "%s: out overlaps q", fn);
    for (const void* v : {sp, zs}) {  // one value per point, contiguous
        lo = reinterpret_cast<uintptr_t>(v), hi = lo + (uintptr_t)n_pts * (uintptr_t)elem;
        ATX_REQUIRE(!(olo < hi && lo < ohi), ATX_EINVAL, "%s: out overlaps %s", fn, v == sp ? "sp" : "zs");
    }
    PltzCall c;
    c.t = t, c.q = q, c.sp = sp, c.zs = zs, c.out = out;
    c.A = A, c.B = B, c.targets = targets;
    c.n_pts = n_pts, c.t_pitch = t_pitch, c.q_pitch = q_pitch, c.out_pitch = out_pitch;
    c.n_lev = (int)n_lev, c.n_tgt = (int)n_tgt, c.first = (int)(n_half - 1 - n_lev), c.layout = layout, c.rows = (int)rows;
    c.log = coordinate == ATX_PLTZ_LOG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dtype == ATX_F32 ? pltz_typed<float>(c, s) : pltz_typed<double>(c, s);
}
