// The parcel ascent: atx_parcel_columns (include/atx_parcel.h holds the statement), built into a library of its own,
// lib/libatx_parcel.so — libatx's entry points are a fixed, tested set, as for the other companion libraries.
//
// A parcel that is lifted level by level is a scan: one lane per point, and 137 levels x 10 Newton steps x (a logarithm, an exponential,
// six divisions) in a row on that lane.  The statement therefore solves every level from ln theta_e of the start level and p_k ALONE, and
// a level is a lane's work.  ATX_COLUMNS, a 256-lane workgroup per tile of PT consecutive points, phases between barriers:
//   1. stage    the tile's t and q columns are two runs of PT x pitch elements: stage_columns (atx_column_tile.hpp) copies each into
//               LDS on its own route, 16 bytes per lane where column_route allows; one lane per point converts sp;
//   2. levels   one lane per (point, level): p_k and ln p_k (per point on hybrid levels, ONE row per tile on pressure levels), Tv of
//               the environment, and ln theta_e of the level's own parcel where the most unstable one is asked for;
//   3. start    WAVE-COOPERATIVE, as the column search: lanes are the levels of a column, a column of W = 2^ceil(log2 n) <= 32
//               levels shares its wave with 64 / W - 1 others.  Two ballots give the first and the last level that takes part and
//               whether a NaN lies between them; the most unstable level is a reduction of (ln theta_e, scan index) pairs over the
//               segment by __shfl_xor, "greater, or equal and nearer the ground" being a total order.  The first lane of a segment
//               forms the parcel — r, T_L, ln theta_e, p_L — and leaves it in LDS;
//   4. solve    one lane per (point, level): the dry adiabat, or the Newton steps, and b_k over the level's Tv in LDS.  All the
//               transcendental work of the kernel sits here, on every lane;
//   5. areas    wave-cooperative again, lanes are steps: the two areas of a step from b and ln p of two neighbouring words; the
//               ballot of pos > 0 and its LAST set bit give the first positive step from the ground.  A float64 stack's areas
//               take the place of its staged t and q, which nothing reads any more: no LDS of their own;
//   6. blocks   one lane per (point, block of 8 steps): the two block sums in the statement's order;
//   7. combine  one lane per point adds the block sums and deposits the five outputs in the tile's output run in LDS;
//   8. store    the output run leaves LDS in order, a point's five values next to each other.
// No lane walks a column in HBM.  PT is what fits the LDS budget (tile_points over ParcelCarve; it does not depend on the pitches).
// ATX_FIELDS: one lane per point, the 64 points of a wave consecutive, so every row is read coalesced: the levels that take part, then
// the start level from the ground up, then ONE walk from the start level up with b of the level below, the two block sums and the
// "first positive step seen" flag in registers: the same float64 operations in the same order, the same bits.
// log and exp are this library's own (atx_parcel_math.hpp, 0.54 and 0.61 ulp): an area is b times a difference of two logarithms near
// 11.5, and atx_log / atx_exp at 0.73 / 0.9 ulp left one float64 case outside the rule of twice numpy's error.
// No scratch (profiles/parcel_resources.json).
#include "../../../include/atx_parcel.h"
#include "../atx_column_tile.hpp"
#include "../atx_host.hpp"
#include "atx_parcel_math.hpp"

namespace atx {

constexpr int kParcelBlock = ATX_PARCEL_BLOCK;
constexpr int kParcelMaxLevels = ATX_PARCEL_MAX_LEVELS;
constexpr int kParcelSteps = ATX_PARCEL_NEWTON_STEPS;
constexpr int kParcelOut = ATX_PARCEL_OUTPUTS;
constexpr int kParcelWaves = kTileBlock / kWave;
constexpr double kRd = 287.0597, kRv = 461.5250, kLn1e5 = 11.512925464970229;

// log and exp of the statement: the refined ones of atx_parcel_math.hpp on their domain, atx_log / atx_exp (IEEE specials) beyond it
__device__ __forceinline__ double parcel_log(double x) {
    return (x >= 2.2250738585072014e-308 && x <= 1.7976931348623157e308) ? parcel_log_normal(x) : atx_log(x);
}
__device__ __forceinline__ double parcel_exp(double x) { return (x > -700.0 && x < 700.0) ? parcel_exp_moderate(x) : atx_exp(x); }

// ---- the statement, one IEEE operation at a time ------------------------------------------------------------------------------------
struct Parcel {  // of the start level; s < 0: every output of the point is NaN
    double T, r, p, lnp, TL, pL, lnthe;
    int s, kt;
};

__device__ __forceinline__ double parcel_eps() { return kRd / kRv; }

__device__ __forceinline__ double ln_theta_e(double lnT, double TL, double r, double lnp) {
    const double dry = lnT + (0.2854 * (1.0 - 0.28 * r)) * (kLn1e5 - lnp);
    return dry + ((3.376 / TL - 0.00254) * (1000.0 * r)) * (1.0 + 0.81 * r);
}

__device__ __forceinline__ double mixing_ratio(double q) { return q / (1.0 - q); }

__device__ __forceinline__ double virtual_t(double T, double r) { return (T * (1.0 + r / parcel_eps())) / (1.0 + r); }

// (r, T_L, ln theta_e) of the parcel of a level
__device__ __forceinline__ void parcel_of_level(double T, double q, double p, double lnp, double& r, double& TL, double& lnthe) {
    r = mixing_ratio(q);
    const double e = (p * r) / (parcel_eps() + r);
    const double lnT = parcel_log(T);
    TL = 2840.0 / ((3.5 * lnT - parcel_log(e / 100.0)) - 4.805) + 55.0;
    lnthe = ln_theta_e(lnT, TL, r, lnp);
}

__device__ __forceinline__ double saturation_ratio(double T, double p, double& pe) {
    const double es = 611.21 * parcel_exp((17.502 * (T - 273.16)) / (T - 32.19));
    pe = p - es;
    return (parcel_eps() * es) / pe;
}

__device__ __forceinline__ Parcel parcel_start(double T, double q, double p, double lnp, int s, int kt) {
    Parcel a;
    a.T = T, a.p = p, a.lnp = lnp, a.s = s, a.kt = kt;
    parcel_of_level(T, q, p, lnp, a.r, a.TL, a.lnthe);
    a.pL = p * parcel_exp(3.5 * parcel_log(a.TL / T));
    return a;
}

// b_k of a level above the start level: tv_env is Tv of the environment there.
__device__ __forceinline__ double parcel_buoyancy(const Parcel& a, double pk, double lnpk, double tv_env) {
    double T = a.T * parcel_exp((2.0 / 7.0) * parcel_log(pk / a.p));
    double r = a.r;
    if (!(pk >= a.pL)) {
        const double lh = parcel_log(pk / 1222.42);
        const double cap = (32.19 * lh - 4780.84632) / (lh - 17.502);
        const double dlp = kLn1e5 - lnpk;
#pragma unroll 1
        for (int it = 0; it < kParcelSteps; ++it) {
            double pe;
            r = saturation_ratio(T, pk, pe);
            const double F = ln_theta_e(parcel_log(T), T, r, lnpk) - a.lnthe;
            const double d = T - 32.19;
            const double dr = (r * (pk / pe)) * (4217.45694 / (d * d));
            const double w = (1000.0 * r) * (1.0 + 0.81 * r);
            const double dF = ((1.0 / T - (0.079912 * dr) * dlp) - (3.376 / (T * T)) * w) + ((3.376 / T - 0.00254) * (1000.0 * dr)) * (1.0 + 1.62 * r);
            const double Tn = T - F / dF;
            T = Tn < cap ? Tn : cap;
        }
        double pe;
        r = saturation_ratio(T, pk, pe);
    }
    return kRd * (virtual_t(T, r) - tv_env);
}

// The two areas of a step between b = lo (the lower level) and hi (the upper), dl = ln p_lower - ln p_upper.
__device__ __forceinline__ void step_areas(double lo, double hi, double dl, double& pos, double& neg) {
    if ((lo > 0.0 && hi < 0.0) || (lo < 0.0 && hi > 0.0)) {
        const double f = lo / (lo - hi);
        const double a_lo = ((lo * f) * dl) / 2.0, a_hi = ((hi * (1.0 - f)) * dl) / 2.0;
        pos = lo > 0.0 ? a_lo : a_hi;
        neg = lo > 0.0 ? a_hi : a_lo;
    } else {
        const double area = ((lo + hi) / 2.0) * dl;
        pos = area > 0.0 ? area : 0.0;
        neg = area > 0.0 ? 0.0 : area;
    }
}

template <int MODE>
__device__ __forceinline__ double level_pressure(const double* __restrict__ A, const double* __restrict__ B, const double* __restrict__ P, int k, double sp) {
    if constexpr (MODE == ATX_PARCEL_HYBRID)
        return full_level(A, B, k, sp);
    else
        return P[k];
}

template <int MODE>
__device__ __forceinline__ bool takes_part(double pk, double sp, double top) {
    return pk >= top && (MODE == ATX_PARCEL_HYBRID || pk <= sp);
}

template <typename T>
__device__ __forceinline__ T parcel_output(int o, bool failed, double cape, double cin, bool found, const Parcel& a) {
    if (failed) return quiet_nan<T>();
    if (o == 1 && !found) return quiet_nan<T>();
    const double y = o == 0 ? cape : o == 1 ? cin : o == 2 ? a.pL : o == 3 ? a.TL : a.p;
    return (T)y;
}

// Where the LDS of a tile of `pt` points holds what (byte offsets, multiples of 16): one definition for the launch and the kernel.
// `cov`: n_lev rounded up to whole 16-byte vectors, the most a staged column takes on either route.
struct ParcelCarve {
    int64_t qs, ps, lps, bs, th, ar, blk, rec, irec, ys, total;  // (the staged t columns start at 0)
};
__host__ __device__ inline ParcelCarve parcel_carve(int64_t pt, int cov, int elem, int n_lev, int mode, int parcel) {
    const int nb = (n_lev + kParcelBlock - 1) / kParcelBlock;
    const int64_t p_rows = mode == ATX_PARCEL_HYBRID ? pt : 1;
    ParcelCarve c;
    c.qs = round16(pt * cov * elem);                                        // T [pt][cov]
    c.ps = c.qs + round16(pt * cov * elem);                                 // double [p_rows][n_lev]
    c.lps = c.ps + round16(p_rows * n_lev * 8);                             // double [p_rows][n_lev]
    c.bs = c.lps + round16(p_rows * n_lev * 8);                             // double [pt][n_lev]: Tv of the environment, then b
    c.th = c.bs + round16(pt * n_lev * 8);                                  // double [pt][n_lev], the most unstable parcel only
    c.ar = c.th + (parcel == ATX_PARCEL_MOST_UNSTABLE ? round16(pt * n_lev * 8) : 0);  // double [2][pt][n_lev], a float32 stack only
    c.blk = c.ar + (elem == 8 ? 0 : round16(2 * pt * n_lev * 8));           // double [pt][2][nb]
    c.rec = c.blk + round16(pt * 2 * nb * 8);                               // double [pt][8]: T, r, p, ln p, T_L, p_L, ln theta_e, sp
    c.irec = c.rec + round16(pt * 64);                                      // int [pt][4]: s, kt, first
    c.ys = c.irec + round16(pt * 16);                                       // T [pt][kParcelOut]
    c.total = c.ys + round16(pt * kParcelOut * elem);
    return c;
}

static inline int parcel_segment(int n_lev) {
    int w = 1;
    while (w < n_lev && w < kWave) w *= 2;
    return w;
}

__device__ __forceinline__ Parcel load_parcel(const double* rec, const int* irec, int pt) {
    const double* r = rec + pt * 8;
    Parcel a;
    a.T = r[0], a.r = r[1], a.p = r[2], a.lnp = r[3], a.TL = r[4], a.pL = r[5], a.lnthe = r[6];
    a.s = irec[pt * 4], a.kt = irec[pt * 4 + 1];
    return a;
}

// ---- ATX_COLUMNS ---------------------------------------------------------------------------------------------------------------------
// VT, VQ: elements per load when t and q are staged (Vec16<T>::N, or 1 for an odd pitch or an unaligned base); t_lds, q_lds: elements
// between the columns of two points in LDS (column_route); cov: the carve's column length; W: the lanes of a segment, log2W its logarithm.
template <typename T, int VT, int VQ, int MODE, int PARCEL>
__global__ void __launch_bounds__(kTileBlock)
parcel_columns_kernel(const T* __restrict__ t, const T* __restrict__ q, const T* __restrict__ sp, T* __restrict__ out, const double* __restrict__ A,
                      const double* __restrict__ B, const double* __restrict__ P, int64_t n_pts, int n_lev, int64_t t_pitch, int64_t q_pitch,
                      int64_t out_pitch, double depth, double top, int PT, int t_lds, int q_lds, int cov, int W, int log2W) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const ParcelCarve lds = parcel_carve(PT, cov, (int)sizeof(T), n_lev, MODE, PARCEL);
    const int nb = (n_lev + kParcelBlock - 1) / kParcelBlock;
    T* ts = reinterpret_cast<T*>(smem);
    T* qs = reinterpret_cast<T*>(smem + lds.qs);
    double* ps = reinterpret_cast<double*>(smem + lds.ps);
    double* lps = reinterpret_cast<double*>(smem + lds.lps);
    double* bs = reinterpret_cast<double*>(smem + lds.bs);
    double* th = reinterpret_cast<double*>(smem + lds.th);
    double* blk = reinterpret_cast<double*>(smem + lds.blk);
    double* rec = reinterpret_cast<double*>(smem + lds.rec);
    int* irec = reinterpret_cast<int*>(smem + lds.irec);
    T* ys = reinterpret_cast<T*>(smem + lds.ys);
    // the areas: in place of the staged t (pos) and q (neg) of a float64 stack, in words of their own for a float32 stack
    constexpr bool kAlias = sizeof(T) == 8;
    double* pos = kAlias ? reinterpret_cast<double*>(smem) : reinterpret_cast<double*>(smem + lds.ar);
    double* neg = kAlias ? reinterpret_cast<double*>(smem + lds.qs) : pos + (int64_t)PT * n_lev;
    const int a_pitch = kAlias ? cov : n_lev;
    const int p_pitch = MODE == ATX_PARCEL_HYBRID ? n_lev : 0;  // (pressure levels: one row for the tile)

    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1), wave = tid >> 6;
    const int G = kWave >> log2W, g = lane >> log2W, j = lane & (W - 1);
    const unsigned long long segment = W == kWave ? ~0ull : ((1ull << W) - 1ull);
    const int64_t p0 = (int64_t)blockIdx.x * PT;
    const int npt = (int)(n_pts - p0 < PT ? n_pts - p0 : PT);
    const int chunks = (n_lev + kWave - 1) / kWave, groups = (npt + G - 1) / G;

    // 1. stage
    stage_columns<T, VT>(t, ts, p0, npt, t_pitch, t_lds, tid);
    stage_columns<T, VQ>(q, qs, p0, npt, q_pitch, q_lds, tid);
    for (int pt = tid; pt < npt; pt += kTileBlock) rec[pt * 8 + 7] = (double)sp[p0 + pt];
    __syncthreads();
    // 2. levels (pressure levels: the tile's one row of p and ln p first, a logarithm per level and not per (point, level))
    if constexpr (MODE == ATX_PARCEL_PRESSURE) {
        for (int k = tid; k < n_lev; k += kTileBlock) ps[k] = P[k], lps[k] = parcel_log(P[k]);
        __syncthreads();
    }
    {
        TileWalk w(tid, n_lev);
        for (int i = tid; i < npt * n_lev; i += kTileBlock, w.next()) {
            const int pt = w.row, k = w.col;
            double pk, lnpk;
            if constexpr (MODE == ATX_PARCEL_HYBRID) {
                pk = full_level(A, B, k, rec[pt * 8 + 7]), lnpk = parcel_log(pk);
                ps[pt * p_pitch + k] = pk, lps[pt * p_pitch + k] = lnpk;
            } else {
                pk = ps[k], lnpk = lps[k];
            }
            const double Tk = (double)ts[(int64_t)pt * t_lds + k], qk = (double)qs[(int64_t)pt * q_lds + k];
            bs[pt * n_lev + k] = virtual_t(Tk, mixing_ratio(qk));
            if constexpr (PARCEL == ATX_PARCEL_MOST_UNSTABLE) {
                double r, TL, lnthe;
                parcel_of_level(Tk, qk, pk, lnpk, r, TL, lnthe);
                th[pt * n_lev + k] = lnthe;
            }
        }
    }
    __syncthreads();
    // 3. start: wave `wave` takes the groups wave, wave + 4, ... of G points; every branch around a ballot or a shuffle is uniform
    for (int grp = wave; grp < groups; grp += kParcelWaves) {
        const int pt = grp * G + g;
        const bool live = pt < npt;
        const int row = live ? pt : 0;
        const double s = rec[row * 8 + 7];
        const double* pp = ps + row * p_pitch;
        int kt = -1, kb = -1;
        bool any_nan = false;
        for (int c = 0; c < chunks; ++c) {
            const int m = c * kWave + j;
            bool part = false, nan = false;
            if (live && m < n_lev) {
                part = takes_part<MODE>(pp[m], s, top);
                const T tv = ts[(int64_t)row * t_lds + m], qv = qs[(int64_t)row * q_lds + m];
                nan = part && (tv != tv || qv != qv);
            }
            const unsigned long long mask = (__ballot(part) >> (g << log2W)) & segment;
            any_nan = any_nan || ((__ballot(nan) >> (g << log2W)) & segment) != 0ull;
            if (mask != 0ull) {
                if (kt < 0) kt = c * kWave + __ffsll((long long)mask) - 1;
                kb = c * kWave + 63 - __clzll((long long)mask);
            }
        }
        int start = kb;
        if constexpr (PARCEL == ATX_PARCEL_MOST_UNSTABLE) {
            const double floor = kb >= 0 ? pp[kb] - depth : 0.0;
            double bv = 0.0;
            int bk = -1;  // the scan index from the ground, kb - k
            for (int c = 0; c < chunks; ++c) {
                const int m = c * kWave + j;
                if (live && kb >= 0 && m >= kt && m <= kb && pp[m] >= floor) {
                    const double v = th[row * n_lev + m];
                    const int k = kb - m;
                    if (bk < 0 || v > bv || (v == bv && k < bk)) bv = v, bk = k;
                }
            }
            for (int offset = W >> 1; offset > 0; offset >>= 1) {
                const double ov = __shfl_xor(bv, offset);
                const int ok = __shfl_xor(bk, offset);
                if (ok >= 0 && (bk < 0 || ov > bv || (ov == bv && ok < bk))) bv = ov, bk = ok;
            }
            start = bk < 0 ? -1 : kb - bk;
        }
        if (live && j == 0) {
            const bool failed = s != s || kb < 0 || any_nan || start < 0;
            Parcel a;
            a.s = -1, a.kt = 0;
            if (!failed)
                a = parcel_start((double)ts[(int64_t)pt * t_lds + start], (double)qs[(int64_t)pt * q_lds + start], pp[start], lps[pt * p_pitch + start], start, kt);
            double* r = rec + pt * 8;
            if (!failed) r[0] = a.T, r[1] = a.r, r[2] = a.p, r[3] = a.lnp, r[4] = a.TL, r[5] = a.pL, r[6] = a.lnthe;
            irec[pt * 4] = a.s, irec[pt * 4 + 1] = a.kt, irec[pt * 4 + 2] = -1;
        }
    }
    __syncthreads();
    // 4. solve
    {
        TileWalk w(tid, n_lev);
        for (int i = tid; i < npt * n_lev; i += kTileBlock, w.next()) {
            const int pt = w.row, k = w.col;
            const int s = irec[pt * 4], kt = irec[pt * 4 + 1];
            double b = 0.0;
            if (k >= kt && k < s) b = parcel_buoyancy(load_parcel(rec, irec, pt), ps[pt * p_pitch + k], lps[pt * p_pitch + k], bs[pt * n_lev + k]);
            bs[pt * n_lev + k] = b;
        }
    }
    __syncthreads();
    // 5. areas: lane j of a segment takes the steps 64 c + j, the chunks from the ground up
    for (int grp = wave; grp < groups; grp += kParcelWaves) {
        const int pt = grp * G + g;
        const bool live = pt < npt;
        const int row = live ? pt : 0;
        const int s = irec[row * 4], kt = irec[row * 4 + 1];
        int first = -1;
        for (int c = chunks - 1; c >= 0; --c) {
            const int m = c * kWave + j;
            double ap = 0.0, an = 0.0;
            const bool step = live && m >= kt && m < s;  // (m + 1 <= s < n_lev)
            if (step) step_areas(bs[row * n_lev + m + 1], bs[row * n_lev + m], lps[row * p_pitch + m + 1] - lps[row * p_pitch + m], ap, an);
            if (live && m < n_lev) pos[(int64_t)row * a_pitch + m] = ap, neg[(int64_t)row * a_pitch + m] = an;
            const unsigned long long mask = (__ballot(step && ap > 0.0) >> (g << log2W)) & segment;
            if (first < 0 && mask != 0ull) first = c * kWave + 63 - __clzll((long long)mask);
        }
        if (live && j == 0) irec[pt * 4 + 2] = first;
    }
    __syncthreads();
    // 6. blocks
    {
        TileWalk w(tid, nb);
        for (int i = tid; i < npt * nb; i += kTileBlock, w.next()) {
            const int pt = w.row, k0 = w.col * kParcelBlock, k1 = k0 + kParcelBlock < n_lev ? k0 + kParcelBlock : n_lev;
            const int s = irec[pt * 4], kt = irec[pt * 4 + 1], first = irec[pt * 4 + 2];
            double bp = 0.0, bn = 0.0;
            for (int m = k1 - 1; m >= k0; --m) {
                if (m >= kt && m < s) {
                    const bool below = first >= 0 && (m > first || (m == first && bs[pt * n_lev + m + 1] < 0.0));
                    bp = bp + pos[(int64_t)pt * a_pitch + m];
                    bn = bn + (below ? neg[(int64_t)pt * a_pitch + m] : 0.0);
                }
            }
            blk[(pt * 2) * nb + w.col] = bp, blk[(pt * 2 + 1) * nb + w.col] = bn;
        }
    }
    __syncthreads();
    // 7. combine
    for (int pt = tid; pt < npt; pt += kTileBlock) {
        const Parcel a = load_parcel(rec, irec, pt);
        double cape = 0.0, cin = 0.0;
        for (int m = nb - 1; m >= 0; --m) cape = cape + blk[(pt * 2) * nb + m], cin = cin + blk[(pt * 2 + 1) * nb + m];
        for (int o = 0; o < kParcelOut; ++o) ys[pt * kParcelOut + o] = parcel_output<T>(o, a.s < 0, cape, cin, irec[pt * 4 + 2] >= 0, a);
    }
    __syncthreads();
    // 8. store
    {
        TileWalk w(tid, kParcelOut);
        for (int i = tid; i < npt * kParcelOut; i += kTileBlock, w.next()) out[(p0 + w.row) * out_pitch + w.col] = ys[w.row * kParcelOut + w.col];
    }
}

// ---- ATX_FIELDS ----------------------------------------------------------------------------------------------------------------------
template <typename T, int MODE, int PARCEL>
__global__ void __launch_bounds__(kTileBlock)
parcel_fields_kernel(const T* __restrict__ t, const T* __restrict__ q, const T* __restrict__ sp, T* __restrict__ out, const double* __restrict__ A,
                     const double* __restrict__ B, const double* __restrict__ P, int64_t n_pts, int n_lev, int64_t t_pitch, int64_t q_pitch,
                     int64_t out_pitch, double depth, double top) {
    const int64_t p = (int64_t)blockIdx.x * kTileBlock + threadIdx.x;
    if (p >= n_pts) return;
    const double s = (double)sp[p];
    auto tk = [&](int k) { return (double)t[(int64_t)k * t_pitch + p]; };
    auto qk = [&](int k) { return (double)q[(int64_t)k * q_pitch + p]; };
    int kt = -1, kb = -1;
    for (int k = 0; k < n_lev; ++k)
        if (takes_part<MODE>(level_pressure<MODE>(A, B, P, k, s), s, top)) {
            if (kt < 0) kt = k;
            kb = k;
        }
    bool failed = s != s || kb < 0;
    int start = kb;
    if (!failed) {
        const double floor = level_pressure<MODE>(A, B, P, kb, s) - depth;
        double best = 0.0;
        bool any = false;
        for (int k = kb; k >= kt; --k) {  // from the ground
            const double Tk = tk(k), Qk = qk(k);
            failed = failed || Tk != Tk || Qk != Qk;
            if constexpr (PARCEL == ATX_PARCEL_MOST_UNSTABLE) {
                const double pk = level_pressure<MODE>(A, B, P, k, s);
                if (pk >= floor) {
                    double r, TL, lnthe;
                    parcel_of_level(Tk, Qk, pk, parcel_log(pk), r, TL, lnthe);
                    if (!any || lnthe > best) best = lnthe, start = k, any = true;
                }
            }
        }
    }
    Parcel a;
    a.s = -1, a.kt = 0;
    double cape = 0.0, cin = 0.0;
    bool found = false;
    if (!failed) {
        const double pstart = level_pressure<MODE>(A, B, P, start, s);
        a = parcel_start(tk(start), qk(start), pstart, parcel_log(pstart), start, kt);
        double lo = 0.0, lnp_lo = a.lnp, bp = 0.0, bn = 0.0;
        for (int m = start - 1; m >= kt; --m) {  // step m: the levels m + 1 (lo) and m
            const double pk = level_pressure<MODE>(A, B, P, m, s), lnpk = parcel_log(pk);
            const double hi = parcel_buoyancy(a, pk, lnpk, virtual_t(tk(m), mixing_ratio(qk(m))));
            double ap, an;
            step_areas(lo, hi, lnp_lo - lnpk, ap, an);
            const bool is_first = !found && ap > 0.0;
            const bool below = !found && (!is_first || lo < 0.0);  // (a step before any positive one counts only if one follows: `found` below)
            bp = bp + ap;
            bn = bn + (below ? an : 0.0);
            found = found || is_first;
            if (m % kParcelBlock == 0 || m == kt) cape = cape + bp, cin = cin + bn, bp = 0.0, bn = 0.0;
            lo = hi, lnp_lo = lnpk;
        }
    }
    for (int o = 0; o < kParcelOut; ++o) out[(int64_t)o * out_pitch + p] = parcel_output<T>(o, failed, cape, cin, found, a);
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
struct ParcelCall {
    const void *t, *q, *sp;
    void* out;
    const double *A, *B, *P;
    int64_t n_pts, t_pitch, q_pitch, out_pitch;
    double depth, top;
    int n_lev, layout;
};

template <typename T>
static int parcel_cov(int n_lev) {
    return (n_lev + Vec16<T>::N - 1) / Vec16<T>::N * Vec16<T>::N;
}

static int parcel_tile(int n_lev, int elem, int mode, int parcel) {
    const int cov = elem == 4 ? parcel_cov<float>(n_lev) : parcel_cov<double>(n_lev);
    return tile_points([&](int64_t pt) { return parcel_carve(pt, cov, elem, n_lev, mode, parcel).total; });
}

template <typename T, int MODE, int PARCEL>
static int parcel_typed(const ParcelCall& c, hipStream_t st) {
    const char* fn = "atx_parcel_columns";
    const T* t = static_cast<const T*>(c.t);
    const T* q = static_cast<const T*>(c.q);
    const T* sp = static_cast<const T*>(c.sp);
    T* out = static_cast<T*>(c.out);
    if (c.layout == ATX_FIELDS) {
        hipLaunchKernelGGL((parcel_fields_kernel<T, MODE, PARCEL>), dim3((unsigned)((c.n_pts + kTileBlock - 1) / kTileBlock)), dim3(kTileBlock), 0, st, t, q, sp,
                           out, c.A, c.B, c.P, c.n_pts, c.n_lev, c.t_pitch, c.q_pitch, c.out_pitch, c.depth, c.top);
        ATX_LAUNCH_CHECK("parcel_fields");
        return ATX_OK;
    }
    constexpr int VEC = Vec16<T>::N;
    const int cov = parcel_cov<T>(c.n_lev);
    const ColumnRoute tr = column_route<VEC>(c.t, c.t_pitch, c.n_lev), qr = column_route<VEC>(c.q, c.q_pitch, c.n_lev);
    const int PT = parcel_tile(c.n_lev, (int)sizeof(T), MODE, PARCEL);
    const int64_t one = parcel_carve(1, cov, (int)sizeof(T), c.n_lev, MODE, PARCEL).total;
    ATX_REQUIRE(PT > 0, ATX_ENOTIMPL, "%s: one point's %d levels need %lld bytes of LDS, a workgroup has %lld", fn, c.n_lev, (long long)one,
                (long long)kTileLdsLimit);
    const int64_t tiles = (c.n_pts + PT - 1) / PT;
    const size_t lds = (size_t)parcel_carve(PT, cov, (int)sizeof(T), c.n_lev, MODE, PARCEL).total;
    const int W = parcel_segment(c.n_lev);
    int log2W = 0;
    while ((1 << log2W) < W) ++log2W;
    auto launch = [&](auto vt, auto vq) {
        hipLaunchKernelGGL((parcel_columns_kernel<T, decltype(vt)::value, decltype(vq)::value, MODE, PARCEL>), dim3((unsigned)tiles), dim3(kTileBlock), lds, st,
                           t, q, sp, out, c.A, c.B, c.P, c.n_pts, c.n_lev, c.t_pitch, c.q_pitch, c.out_pitch, c.depth, c.top, PT, tr.lds_pitch, qr.lds_pitch,
                           cov, W, log2W);
        return 0;
    };
    const std::integral_constant<int, VEC> wide{};
    const std::integral_constant<int, 1> single{};
    auto with_width = [&](bool vector, auto&& f) { return vector ? f(wide) : f(single); };
    with_width(tr.vector, [&](auto vt) { return with_width(qr.vector, [&](auto vq) { return launch(vt, vq); }); });
    ATX_LAUNCH_CHECK("parcel_columns");
    return ATX_OK;
}

template <typename T>
static int parcel_dispatch(const ParcelCall& c, int mode, int parcel, hipStream_t s) {
    if (mode == ATX_PARCEL_HYBRID)
        return parcel == ATX_PARCEL_LOWEST ? parcel_typed<T, ATX_PARCEL_HYBRID, ATX_PARCEL_LOWEST>(c, s)
                                           : parcel_typed<T, ATX_PARCEL_HYBRID, ATX_PARCEL_MOST_UNSTABLE>(c, s);
    return parcel == ATX_PARCEL_LOWEST ? parcel_typed<T, ATX_PARCEL_PRESSURE, ATX_PARCEL_LOWEST>(c, s)
                                       : parcel_typed<T, ATX_PARCEL_PRESSURE, ATX_PARCEL_MOST_UNSTABLE>(c, s);
}

// The bytes [lo, hi) that `rows` rows of a stack touch; a per-point vector is one row of a field-major stack.
struct ParcelExtent {
    uintptr_t lo, hi;
    bool overlaps(const ParcelExtent& o) const { return lo < o.hi && o.lo < hi; }
};
static ParcelExtent parcel_extent(const void* base, int64_t n_pts, int64_t rows, int64_t pitch, int layout, int elem) {
    const int64_t elements = layout == ATX_COLUMNS ? (n_pts - 1) * pitch + rows : (rows - 1) * pitch + n_pts;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(base);
    return {lo, lo + (uintptr_t)elements * (uintptr_t)elem};
}

}  // namespace atx

using namespace atx;

extern "C" int atx_parcel_version(void) { return ATX_PARCEL_VERSION; }

extern "C" const char* atx_parcel_last_error(void) { return last_error().c_str(); }

extern "C" int atx_parcel_host_math(const double* x, double* y, int64_t n, int which) {
    ATX_REQUIRE((which == 0 || which == 1) && n >= 0 && ((x && y) || n == 0), ATX_EINVAL, "atx_parcel_host_math: bad arguments (n=%lld, which=%d)", (long long)n, which);
    for (int64_t i = 0; i < n; ++i) y[i] = which == 0 ? parcel_log_normal(x[i]) : parcel_exp_moderate(x[i]);
    return ATX_OK;
}

extern "C" int atx_parcel_tile_points(int64_t n_lev, int dtype, int mode, int parcel) {
    if (n_lev < 1 || n_lev > kParcelMaxLevels || (dtype != ATX_F32 && dtype != ATX_F64)) return 0;
    if ((mode != ATX_PARCEL_HYBRID && mode != ATX_PARCEL_PRESSURE) || (parcel != ATX_PARCEL_LOWEST && parcel != ATX_PARCEL_MOST_UNSTABLE)) return 0;
    return parcel_tile((int)n_lev, dtype == ATX_F32 ? 4 : 8, mode, parcel);
}

extern "C" int atx_parcel_columns(const void* t, const void* q, const void* sp, void* out, const double* A, const double* B, const double* levels_pa,
                                  int64_t n_pts, int64_t n_lev, int64_t t_pitch, int64_t q_pitch, int64_t out_pitch, double depth_pa, double top_pa, int dtype,
                                  int layout, int mode, int parcel, void* stream) {
    const char* fn = "atx_parcel_columns";
    ATX_REQUIRE(dtype == ATX_F32 || dtype == ATX_F64, ATX_EINVAL, "%s: bad dtype %d", fn, dtype);
    ATX_REQUIRE(layout == ATX_COLUMNS || layout == ATX_FIELDS, ATX_EINVAL, "%s: bad layout %d", fn, layout);
    ATX_REQUIRE(mode == ATX_PARCEL_HYBRID || mode == ATX_PARCEL_PRESSURE, ATX_EINVAL, "%s: unknown mode %d", fn, mode);
    ATX_REQUIRE(parcel == ATX_PARCEL_LOWEST || parcel == ATX_PARCEL_MOST_UNSTABLE, ATX_EINVAL, "%s: unknown parcel %d", fn, parcel);
    ATX_REQUIRE(n_pts >= 0 && n_lev >= 1, ATX_EINVAL, "%s: bad sizes n_pts=%lld n_lev=%lld", fn, (long long)n_pts, (long long)n_lev);
    ATX_REQUIRE(top_pa >= 0.0 && depth_pa >= 0.0, ATX_EINVAL, "%s: top_pa = %g and depth_pa = %g must both be >= 0", fn, top_pa, depth_pa);
    ATX_REQUIRE(n_lev <= kParcelMaxLevels, ATX_ENOTIMPL, "%s: n_lev=%lld exceeds the %d levels of one call", fn, (long long)n_lev, kParcelMaxLevels);
    ATX_REQUIRE(n_pts <= INT32_MAX, ATX_ENOTIMPL, "%s: n_pts=%lld exceeds the indexing of one launch", fn, (long long)n_pts);
    if (layout == ATX_COLUMNS) {
        ATX_REQUIRE(t_pitch >= n_lev && q_pitch >= n_lev && out_pitch >= kParcelOut, ATX_ESHAPE, "%s: column pitch (%lld, %lld, %lld) < rows (%lld, %lld, %d)", fn,
                    (long long)t_pitch, (long long)q_pitch, (long long)out_pitch, (long long)n_lev, (long long)n_lev, kParcelOut);
    } else {
        ATX_REQUIRE(t_pitch >= n_pts && q_pitch >= n_pts && out_pitch >= n_pts, ATX_ESHAPE, "%s: field pitch (%lld, %lld, %lld) < points %lld", fn,
                    (long long)t_pitch, (long long)q_pitch, (long long)out_pitch, (long long)n_pts);
    }
    ATX_REQUIRE((t && q && sp && out) || n_pts == 0, ATX_EINVAL, "%s: null t / q / sp / out pointer", fn);
    ATX_REQUIRE(mode != ATX_PARCEL_HYBRID || (A && B) || n_pts == 0, ATX_EINVAL, "%s: null A / B table", fn);
    ATX_REQUIRE(mode != ATX_PARCEL_PRESSURE || levels_pa || n_pts == 0, ATX_EINVAL, "%s: null levels_pa", fn);
    if (n_pts == 0) return ATX_OK;
    const int elem = dtype == ATX_F32 ? 4 : 8;
    const ParcelExtent o = parcel_extent(out, n_pts, kParcelOut, out_pitch, layout, elem);
    ATX_REQUIRE(!o.overlaps(parcel_extent(t, n_pts, n_lev, t_pitch, layout, elem)), ATX_EINVAL, "%s: out overlaps t", fn);
    ATX_REQUIRE(!o.overlaps(parcel_extent(q, n_pts, n_lev, q_pitch, layout, elem)), ATX_EINVAL, "%s: out overlaps q", fn);
    ATX_REQUIRE(!o.overlaps(parcel_extent(sp, n_pts, 1, n_pts, ATX_FIELDS, elem)), ATX_EINVAL, "%s: out overlaps sp", fn);
    ParcelCall c = {};
    c.t = t, c.q = q, c.sp = sp, c.out = out, c.A = A, c.B = B, c.P = levels_pa;
    c.n_pts = n_pts, c.t_pitch = t_pitch, c.q_pitch = q_pitch, c.out_pitch = out_pitch, c.depth = depth_pa, c.top = top_pa;
    c.n_lev = (int)n_lev, c.layout = layout;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dtype == ATX_F32 ? parcel_dispatch<float>(c, mode, parcel, s) : parcel_dispatch<double>(c, mode, parcel, s);
}
