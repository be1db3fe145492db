// Column integrals and layer means: atx_integral_columns (include/atx_integral.h holds the statement), built into a library of its own,
// lib/libatx_integral.so — libatx's entry points are a fixed, tested set, as for the other companion libraries.
//
// The other vertical kernels move values between levels; this one REDUCES a column, and the order of a float64 sum is part of its
// statement.  A running sum down the column is one lane per point (the geopotential scan): a tile of 9 points x 137 levels would keep 9
// of 256 lanes busy.  The statement's sum is therefore BLOCKED — ATX_INTEGRAL_BLOCK consecutive levels into a block sum, the block sums
// into the result — and a block is a lane's work.  ATX_COLUMNS, a 256-lane workgroup per tile of PT consecutive points, five phases:
//   1. stage     the tile's variable columns are one run of PT x pitch elements: stage_columns (atx_column_tile.hpp) copies it into LDS
//                in order, 16 bytes per lane where column_route allows; one lane per point converts sp and, on pressure levels, counts
//                the levels above the ground by bisection in the table; the terms and bounds of the launch go from the kernel
//                arguments into LDS, where a lane can index them;
//   2. weights   one lane per (point, bound, level) evaluates w ONCE, for all terms, into LDS as float64.  On pressure levels a
//                segment feeds two levels: every level's lane computes its OWN two shares (the segment above, the segment below), so
//                no two lanes write one word.  Level k of a (point, bound) sits at word k + k / BLOCK: one float64 of padding per block;
//   3. block sums  one lane per (point, bound, term, block), the block fastest: it walks its BLOCK levels in ascending order, skips
//                w == 0, multiplies and adds in registers and leaves the block sum in LDS; the block lanes of term 0 also sum the
//                weights where a mean is asked for.  Neighbouring lanes read weights BLOCK + 1 float64 apart — 18 words: 16 lanes
//                cover all 32 banks pairwise, no conflict — and values BLOCK elements apart: in float32 the 18 block lanes of a
//                (point, term) share 4 banks, and what spreads a wave over the others is the lanes of the other terms and points,
//                whose columns start n_lev and pitch elements further on — 137 levels are odd, so 3 terms reach 24 banks; a
//                power-of-two n_lev would leave every lane of a wave on those 4.  The values are staged as they lie in memory (one
//                16-byte copy, no padding), so this phase keeps those conflicts;
//   4. combine   one lane per (point, bound, term) adds the block sums in ascending order, divides by g or by the weight sum, rounds
//                once and deposits into the tile's output run in LDS;
//   5. store     the output run leaves LDS in order: 16 bytes per lane where out allows, single elements otherwise.
// No lane walks a column in HBM.  PT is what fits the LDS budget of the launch (tile_points over IntegralCarve).
// ATX_FIELDS: one lane per (point, bound), the 64 points of a wave consecutive, so every row is read coalesced; the lane walks the terms,
// and for each the levels, with the block sum and the result in registers: the same float64 operations in the same order, the same
// bits.  No scratch (profiles/integral_resources.json).
#include "../../../include/atx_integral.h"
#include "../atx_column_tile.hpp"

namespace atx {

constexpr int kIntegralBlock = ATX_INTEGRAL_BLOCK;
constexpr int kIntegralMaxLevels = ATX_INTEGRAL_MAX_LEVELS;
constexpr int kIntegralMaxTerms = ATX_INTEGRAL_MAX_TERMS;
constexpr int kIntegralMaxBounds = ATX_INTEGRAL_MAX_BOUNDS;

// What travels with the launch: the validated host arrays of the call.
struct IntegralSpec {
    double bounds[kIntegralMaxBounds][2];
    int16_t v1[kIntegralMaxTerms], v2[kIntegralMaxTerms];
};

// ---- the statement's weights, one IEEE operation at a time ------------------------------------------------------------------------------
__device__ __forceinline__ double clipped(double a, double c) { return c > a ? c - a : 0.0; }

__device__ __forceinline__ double hybrid_weight(const double* __restrict__ A, const double* __restrict__ B, int k, double sp, double top, double bottom) {
    const double lo = half_level(A, B, k, sp), hi = half_level(A, B, k + 1, sp);
    const double a = lo > top ? lo : top;
    const double c = hi < bottom ? hi : bottom;
    return clipped(a, c);
}

// m = #{k : P[k] <= sp} (a NaN sp counts nothing): the first k with P[k] > sp of a strictly increasing table.
__device__ __forceinline__ int levels_above_ground(const double* __restrict__ P, int n, double sp) {
    int m = 0, hi = n;
    while (m < hi) {
        const int mid = (m + hi) >> 1;
        if (P[mid] <= sp)
            m = mid + 1;
        else
            hi = mid;
    }
    return m;
}

// The share of segment [pj, pn], clipped to the bound, that goes to its LOWER end pn (r) and to its UPPER end pj (1 - r).
__device__ __forceinline__ double segment_share(double pj, double pn, double top, double bottom, bool to_lower_end) {
    const double a = pj > top ? pj : top;
    const double c = pn < bottom ? pn : bottom;
    if (!(c > a)) return 0.0;
    const double len = c - a;
    const double sum = a + c;
    const double mid = sum / 2.0;
    const double num = mid - pj, den = pn - pj;
    const double r = num / den;  // IEEE division
    if (to_lower_end) return len * r;
    const double rest = 1.0 - r;
    return len * rest;
}

__device__ __forceinline__ double pressure_weight(const double* __restrict__ P, int k, int m, double sp, double top, double bottom) {
    if (k >= m) return 0.0;
    const double pk = P[k];
    const double above = k >= 1 ? segment_share(P[k - 1], pk, top, bottom, true) : 0.0;
    double below;
    if (k + 1 < m) {
        below = segment_share(pk, P[k + 1], top, bottom, false);
    } else {  // the lowest level above the ground holds its value down to the ground
        const double a = pk > top ? pk : top;
        const double c = sp < bottom ? sp : bottom;
        below = clipped(a, c);
    }
    return above + below;
}

template <int MODE>
__device__ __forceinline__ double level_weight(const double* __restrict__ A, const double* __restrict__ B, const double* __restrict__ P, int k, int m,
                                               double sp, double top, double bottom) {
    if constexpr (MODE == ATX_INTEGRAL_HYBRID)
        return hybrid_weight(A, B, k, sp, top, bottom);
    else
        return pressure_weight(P, k, m, sp, top, bottom);
}

// acc / g, or acc / wsum; a NaN sp: NaN.  Rounded once to T.
template <typename T>
__device__ __forceinline__ T integral_result(double acc, double wsum, double sp, int kind) {
    if (sp != sp) return quiet_nan<T>();
    const double y = kind == ATX_INTEGRAL_MEAN ? acc / wsum : acc / ATX_INTEGRAL_G;
    return (T)y;
}

// Where level k of a (point, bound) sits in its padded weight row, and the length of such a row (float64 words).
__host__ __device__ inline int padded(int k) { return k + k / kIntegralBlock; }

// Where the LDS of a tile of `pt` points holds what (byte offsets, multiples of 16): one definition for the launch and the kernel.
struct IntegralCarve {
    int64_t ws, bs, sp, ys, m, spec, total;  // (the staged variable columns start at 0)
};
__host__ __device__ inline IntegralCarve integral_carve(int64_t pt, int x_pitch, int elem, int n_lev, int n_term, int n_bnd, int sums) {
    const int nb = (n_lev + kIntegralBlock - 1) / kIntegralBlock;
    IntegralCarve c;
    c.ws = round16(pt * x_pitch * elem);                          // double [pt][n_bnd][padded(n_lev)]
    c.bs = c.ws + round16(pt * n_bnd * padded(n_lev) * 8);         // double [pt][n_bnd][sums][nb]
    c.sp = c.bs + round16(pt * n_bnd * sums * nb * 8);             // double [pt]
    c.ys = c.sp + round16(pt * 8);                                 // T [pt][n_term * n_bnd]
    c.m = c.ys + round16(pt * n_term * n_bnd * elem);              // int [pt]
    c.spec = c.m + round16(pt * 4);                                // double [n_bnd][2], int [n_term][2]
    c.total = c.spec + round16(n_bnd * 16) + round16(n_term * 8);
    return c;
}

// ---- ATX_COLUMNS ---------------------------------------------------------------------------------------------------------------------
// VX: elements per load when the columns are staged (Vec16<T>::N, or 1 for an odd pitch or an unaligned base); VO: elements per store
// of the output run; x_pitch: elements between the columns of two points in LDS (column_route).
template <typename T, int VX, int VO, int MODE>
__global__ void __launch_bounds__(kTileBlock)
integral_columns_kernel(const T* __restrict__ src, const T* __restrict__ sp, T* __restrict__ out, const double* __restrict__ A, const double* __restrict__ B,
                        const double* __restrict__ P, const IntegralSpec spec, int64_t n_pts, int n_lev, int n_term, int n_bnd, int64_t src_pitch,
                        int64_t out_pitch, int PT, int x_pitch, int kind) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int per_point = n_term * n_bnd;
    const int sums = n_term + (kind == ATX_INTEGRAL_MEAN ? 1 : 0);  // (the last row of block sums is the weights' own)
    const int nb = (n_lev + kIntegralBlock - 1) / kIntegralBlock, w_row = padded(n_lev);
    const IntegralCarve lds = integral_carve(PT, x_pitch, (int)sizeof(T), n_lev, n_term, n_bnd, sums);
    const T* xs = reinterpret_cast<const T*>(smem);
    double* ws = reinterpret_cast<double*>(smem + lds.ws);
    double* bs = reinterpret_cast<double*>(smem + lds.bs);
    double* sps = reinterpret_cast<double*>(smem + lds.sp);
    T* ys = reinterpret_cast<T*>(smem + lds.ys);
    int* ms = reinterpret_cast<int*>(smem + lds.m);
    double* bnd = reinterpret_cast<double*>(smem + lds.spec);
    int* trm = reinterpret_cast<int*>(smem + lds.spec + round16(n_bnd * 16));

    const int tid = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * PT;
    const int npt = (int)(n_pts - p0 < PT ? n_pts - p0 : PT);

    // 1. stage
    stage_columns<T, VX>(src, reinterpret_cast<T*>(smem), p0, npt, src_pitch, x_pitch, tid);
    for (int pt = tid; pt < npt; pt += kTileBlock) {
        const double s = (double)sp[p0 + pt];
        sps[pt] = s;
        if constexpr (MODE == ATX_INTEGRAL_PRESSURE) ms[pt] = levels_above_ground(P, n_lev, s);
    }
    for (int b = 0; b < n_bnd; ++b)  // (a uniform index into the kernel arguments; one lane writes)
        if (tid == 0) bnd[2 * b] = spec.bounds[b][0], bnd[2 * b + 1] = spec.bounds[b][1];
    for (int t = 0; t < n_term; ++t)
        if (tid == 0) trm[2 * t] = spec.v1[t], trm[2 * t + 1] = spec.v2[t];
    __syncthreads();
    // 2. weights
    {
        TileWalk w(tid, n_bnd * n_lev);
        for (int i = tid; i < npt * n_bnd * n_lev; i += kTileBlock, w.next()) {
            const int pt = w.row, b = w.col / n_lev, k = w.col - b * n_lev;
            const int m = MODE == ATX_INTEGRAL_PRESSURE ? ms[pt] : 0;
            ws[((int64_t)pt * n_bnd + b) * w_row + padded(k)] = level_weight<MODE>(A, B, P, k, m, sps[pt], bnd[2 * b], bnd[2 * b + 1]);
        }
    }
    __syncthreads();
    // 3. block sums
    {
        const int width = n_bnd * n_term * nb;
        TileWalk w(tid, width);
        for (int i = tid; i < npt * width; i += kTileBlock, w.next()) {
            const int pt = w.row, bt = w.col / nb, blk = w.col - bt * nb;
            const int b = bt / n_term, t = bt - b * n_term;
            const int v1 = trm[2 * t], v2 = trm[2 * t + 1];
            const int k0 = blk * kIntegralBlock, k1 = k0 + kIntegralBlock < n_lev ? k0 + kIntegralBlock : n_lev;
            const double* wk = ws + ((int64_t)pt * n_bnd + b) * w_row + padded(k0) - k0;
            const T* x1 = xs + (int64_t)pt * x_pitch + v1 * n_lev;
            const T* x2 = xs + (int64_t)pt * x_pitch + (v2 < 0 ? v1 : v2) * n_lev;
            double sum = 0.0, wsum = 0.0;
            for (int k = k0; k < k1; ++k) {
                const double wt = wk[k];
                if (wt != 0.0) {
                    double f = (double)x1[k];
                    if (v2 >= 0) f = f * (double)x2[k];
                    const double term = wt * f;
                    sum = sum + term;
                    wsum = wsum + wt;
                }
            }
            double* row = bs + ((int64_t)pt * n_bnd + b) * sums * nb;
            row[t * nb + blk] = sum;
            if (t == 0 && kind == ATX_INTEGRAL_MEAN) row[n_term * nb + blk] = wsum;
        }
    }
    __syncthreads();
    // 4. combine
    {
        TileWalk w(tid, per_point);
        for (int i = tid; i < npt * per_point; i += kTileBlock, w.next()) {
            const int pt = w.row, b = w.col / n_term, t = w.col - b * n_term;
            const double* row = bs + ((int64_t)pt * n_bnd + b) * sums * nb;
            double acc = 0.0, wsum = 0.0;
            for (int blk = 0; blk < nb; ++blk) acc = acc + row[t * nb + blk];
            if (kind == ATX_INTEGRAL_MEAN)
                for (int blk = 0; blk < nb; ++blk) wsum = wsum + row[n_term * nb + blk];
            ys[(int64_t)pt * per_point + t * n_bnd + b] = integral_result<T>(acc, wsum, sps[pt], kind);
        }
    }
    __syncthreads();
    // 5. store (VO > 1: per_point and out_pitch are multiples of VO and out is 16-byte aligned)
    {
        const int C = per_point / VO;
        TileWalk w(tid, C);
        for (int i = tid; i < npt * C; i += kTileBlock, w.next()) {
            const Pack<T, VO> v = *reinterpret_cast<const Pack<T, VO>*>(ys + (int64_t)w.row * per_point + w.col * VO);
            *reinterpret_cast<Pack<T, VO>*>(out + (p0 + w.row) * out_pitch + (int64_t)w.col * VO) = v;
        }
    }
}

// ---- ATX_FIELDS ----------------------------------------------------------------------------------------------------------------------
template <typename T, int MODE>
__global__ void __launch_bounds__(kTileBlock)
integral_fields_kernel(const T* __restrict__ src, const T* __restrict__ sp, T* __restrict__ out, const double* __restrict__ A, const double* __restrict__ B,
                       const double* __restrict__ P, const IntegralSpec spec, int64_t n_pts, int n_lev, int n_term, int n_bnd, int64_t src_pitch,
                       int64_t out_pitch, int kind) {
    const int64_t p = (int64_t)blockIdx.x * kTileBlock + threadIdx.x;
    if (p >= n_pts) return;
    const int b = blockIdx.y;
    const double s = (double)sp[p], top = spec.bounds[b][0], bottom = spec.bounds[b][1];
    const int m = MODE == ATX_INTEGRAL_PRESSURE ? levels_above_ground(P, n_lev, s) : 0;
    for (int t = 0; t < n_term; ++t) {  // (uniform: the kernel arguments are indexed by scalars)
        const int v1 = spec.v1[t], v2 = spec.v2[t];
        const T* x1 = src + (int64_t)v1 * n_lev * src_pitch + p;
        const T* x2 = src + (int64_t)(v2 < 0 ? v1 : v2) * n_lev * src_pitch + p;
        double acc = 0.0, wacc = 0.0;
        for (int k0 = 0; k0 < n_lev; k0 += kIntegralBlock) {
            const int k1 = k0 + kIntegralBlock < n_lev ? k0 + kIntegralBlock : n_lev;
            double sum = 0.0, wsum = 0.0;
            for (int k = k0; k < k1; ++k) {
                const double wt = level_weight<MODE>(A, B, P, k, m, s, top, bottom);
                if (wt != 0.0) {
                    double f = (double)x1[(int64_t)k * src_pitch];
                    if (v2 >= 0) f = f * (double)x2[(int64_t)k * src_pitch];
                    const double term = wt * f;
                    sum = sum + term;
                    wsum = wsum + wt;
                }
            }
            acc = acc + sum;
            wacc = wacc + wsum;
        }
        out[((int64_t)t * n_bnd + b) * out_pitch + p] = integral_result<T>(acc, wacc, s, kind);
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
struct IntegralCall {
    const void *src, *sp;
    void* out;
    const double *A, *B, *P;
    IntegralSpec spec;
    int64_t n_pts, src_pitch, out_pitch;
    int n_var, n_lev, n_term, n_bnd, layout, mode, kind;
};

template <typename T, int MODE>
static int integral_typed(const IntegralCall& c, hipStream_t st) {
    const char* fn = "atx_integral_columns";
    const T* src = static_cast<const T*>(c.src);
    const T* sp = static_cast<const T*>(c.sp);
    T* out = static_cast<T*>(c.out);
    if (c.layout == ATX_FIELDS) {
        const dim3 grid((unsigned)((c.n_pts + kTileBlock - 1) / kTileBlock), (unsigned)c.n_bnd);
        hipLaunchKernelGGL((integral_fields_kernel<T, MODE>), grid, dim3(kTileBlock), 0, st, src, sp, out, c.A, c.B, c.P, c.spec, c.n_pts, c.n_lev, c.n_term,
                           c.n_bnd, c.src_pitch, c.out_pitch, c.kind);
        ATX_LAUNCH_CHECK("integral_fields");
        return ATX_OK;
    }
    constexpr int VEC = Vec16<T>::N;
    const int rows = c.n_var * c.n_lev, per_point = c.n_term * c.n_bnd, sums = c.n_term + (c.kind == ATX_INTEGRAL_MEAN ? 1 : 0);
    const ColumnRoute xr = column_route<VEC>(c.src, c.src_pitch, rows);
    const bool out_vector = aligned16(c.out) && c.out_pitch % VEC == 0 && per_point % VEC == 0;
    auto bytes = [&](int64_t pt) { return integral_carve(pt, xr.lds_pitch, (int)sizeof(T), c.n_lev, c.n_term, c.n_bnd, sums).total; };
    const int PT = tile_points(bytes);
    ATX_REQUIRE(PT > 0, ATX_ENOTIMPL, "%s: one point's %d rows, %d x %d weights and %d x %d block sums need %lld bytes of LDS, a workgroup has %lld", fn, rows,
                c.n_bnd, c.n_lev, c.n_bnd, sums, (long long)bytes(1), (long long)kTileLdsLimit);
    const int64_t tiles = (c.n_pts + PT - 1) / PT;
    const size_t lds = (size_t)bytes(PT);
    auto launch = [&](auto vx, auto vo) {
        hipLaunchKernelGGL((integral_columns_kernel<T, decltype(vx)::value, decltype(vo)::value, MODE>), dim3((unsigned)tiles), dim3(kTileBlock), lds, st, src,
                           sp, out, c.A, c.B, c.P, c.spec, c.n_pts, c.n_lev, c.n_term, c.n_bnd, c.src_pitch, c.out_pitch, PT, xr.lds_pitch, c.kind);
        return 0;
    };
    const std::integral_constant<int, VEC> wide{};
    const std::integral_constant<int, 1> one{};
    auto with_width = [&](bool vector, auto&& f) { return vector ? f(wide) : f(one); };
    with_width(xr.vector, [&](auto vx) { return with_width(out_vector, [&](auto vo) { return launch(vx, vo); }); });
    ATX_LAUNCH_CHECK("integral_columns");
    return ATX_OK;
}

// The bytes [lo, hi) that `rows` rows of a stack touch; a per-point vector is one row of a field-major stack.
struct IntegralExtent {
    uintptr_t lo, hi;
    bool overlaps(const IntegralExtent& o) const { return lo < o.hi && o.lo < hi; }
};
static IntegralExtent integral_extent(const void* base, int64_t n_pts, int64_t rows, int64_t pitch, int layout, int elem) {
    const int64_t elements = layout == ATX_COLUMNS ? (n_pts - 1) * pitch + rows : (rows - 1) * pitch + n_pts;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(base);
    return {lo, lo + (uintptr_t)elements * (uintptr_t)elem};
}

}  // namespace atx

using namespace atx;

extern "C" int atx_integral_version(void) { return ATX_INTEGRAL_VERSION; }

extern "C" const char* atx_integral_last_error(void) { return last_error().c_str(); }

extern "C" int atx_integral_columns(const void* src, const void* sp, void* out, const int32_t* terms, const double* bounds, const double* A, const double* B,
                                    const double* levels_pa, int64_t n_pts, int64_t n_var, int64_t n_lev, int64_t n_term, int64_t n_bnd, int64_t src_pitch,
                                    int64_t out_pitch, int dtype, int layout, int mode, int kind, void* stream) {
    const char* fn = "atx_integral_columns";
    ATX_REQUIRE(dtype == ATX_F32 || dtype == ATX_F64, ATX_EINVAL, "%s: bad dtype %d", fn, dtype);
    ATX_REQUIRE(layout == ATX_COLUMNS || layout == ATX_FIELDS, ATX_EINVAL, "%s: bad layout %d", fn, layout);
    ATX_REQUIRE(mode == ATX_INTEGRAL_HYBRID || mode == ATX_INTEGRAL_PRESSURE, ATX_EINVAL, "%s: unknown mode %d", fn, mode);
    ATX_REQUIRE(kind == ATX_INTEGRAL_SUM || kind == ATX_INTEGRAL_MEAN, ATX_EINVAL, "%s: unknown kind %d", fn, kind);
    ATX_REQUIRE(n_pts >= 0 && n_var >= 1 && n_lev >= 1 && n_term >= 0 && n_bnd >= 0, ATX_EINVAL,
                "%s: bad sizes n_pts=%lld n_var=%lld n_lev=%lld n_term=%lld n_bnd=%lld", fn, (long long)n_pts, (long long)n_var, (long long)n_lev,
                (long long)n_term, (long long)n_bnd);
    ATX_REQUIRE(n_lev <= kIntegralMaxLevels, ATX_ENOTIMPL, "%s: n_lev=%lld exceeds the %d levels of one call", fn, (long long)n_lev, kIntegralMaxLevels);
    ATX_REQUIRE(n_term <= kIntegralMaxTerms && n_bnd <= kIntegralMaxBounds, ATX_ENOTIMPL, "%s: n_term=%lld, n_bnd=%lld exceed the %d terms and %d bounds of one call",
                fn, (long long)n_term, (long long)n_bnd, kIntegralMaxTerms, kIntegralMaxBounds);
    ATX_REQUIRE(n_pts <= INT32_MAX && n_var <= 32767 && n_var * n_lev <= 65535, ATX_ENOTIMPL,
                "%s: sizes exceed the indexing of one launch (n_pts=%lld n_var=%lld n_lev=%lld)", fn, (long long)n_pts, (long long)n_var, (long long)n_lev);
    if (layout == ATX_COLUMNS) {
        ATX_REQUIRE(src_pitch >= n_var * n_lev && out_pitch >= n_term * n_bnd, ATX_ESHAPE, "%s: column pitch (%lld, %lld) < rows (%lld, %lld)", fn,
                    (long long)src_pitch, (long long)out_pitch, (long long)(n_var * n_lev), (long long)(n_term * n_bnd));
    } else {
        ATX_REQUIRE(src_pitch >= n_pts && out_pitch >= n_pts, ATX_ESHAPE, "%s: field pitch (%lld, %lld) < points %lld", fn, (long long)src_pitch,
                    (long long)out_pitch, (long long)n_pts);
    }
    ATX_REQUIRE(terms || n_term == 0, ATX_EINVAL, "%s: null terms", fn);
    ATX_REQUIRE(bounds || n_bnd == 0, ATX_EINVAL, "%s: null bounds", fn);
    IntegralCall c = {};
    for (int64_t t = 0; t < n_term; ++t) {
        const int64_t v1 = terms[2 * t], v2 = terms[2 * t + 1];
        ATX_REQUIRE(v1 >= 0 && v1 < n_var && v2 < n_var, ATX_EINVAL, "%s: terms[%lld] = (%lld, %lld) is outside the %lld variables", fn, (long long)t,
                    (long long)v1, (long long)v2, (long long)n_var);
        c.spec.v1[t] = (int16_t)v1, c.spec.v2[t] = (int16_t)(v2 < 0 ? -1 : v2);
    }
    for (int64_t b = 0; b < n_bnd; ++b) {
        const double top = bounds[2 * b], bottom = bounds[2 * b + 1];
        ATX_REQUIRE(top >= 0.0 && top < bottom, ATX_EINVAL, "%s: bounds[%lld] = (%g, %g) is not 0 <= top < bottom", fn, (long long)b, top, bottom);
        c.spec.bounds[b][0] = top, c.spec.bounds[b][1] = bottom;
    }
    ATX_REQUIRE((src && sp) || n_pts == 0, ATX_EINVAL, "%s: null src / sp pointer", fn);
    ATX_REQUIRE(mode != ATX_INTEGRAL_HYBRID || (A && B) || n_pts == 0, ATX_EINVAL, "%s: null A / B table", fn);
    ATX_REQUIRE(mode != ATX_INTEGRAL_PRESSURE || levels_pa || n_pts == 0, ATX_EINVAL, "%s: null levels_pa", fn);
    ATX_REQUIRE(out || n_pts == 0 || n_term == 0 || n_bnd == 0, ATX_EINVAL, "%s: null out pointer", fn);
    if (n_pts == 0 || n_term == 0 || n_bnd == 0) return ATX_OK;
    const int elem = dtype == ATX_F32 ? 4 : 8;
    const IntegralExtent o = integral_extent(out, n_pts, n_term * n_bnd, out_pitch, layout, elem);
    ATX_REQUIRE(!o.overlaps(integral_extent(src, n_pts, n_var * n_lev, src_pitch, layout, elem)), ATX_EINVAL, "%s: out overlaps src", fn);
    ATX_REQUIRE(!o.overlaps(integral_extent(sp, n_pts, 1, n_pts, ATX_FIELDS, elem)), ATX_EINVAL, "%s: out overlaps sp", fn);
    c.src = src, c.sp = sp, c.out = out, c.A = A, c.B = B, c.P = levels_pa;
    c.n_pts = n_pts, c.src_pitch = src_pitch, c.out_pitch = out_pitch;
    c.n_var = (int)n_var, c.n_lev = (int)n_lev, c.n_term = (int)n_term, c.n_bnd = (int)n_bnd, c.layout = layout, c.mode = mode, c.kind = kind;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (mode == ATX_INTEGRAL_HYBRID) return dtype == ATX_F32 ? integral_typed<float, ATX_INTEGRAL_HYBRID>(c, s) : integral_typed<double, ATX_INTEGRAL_HYBRID>(c, s);
    return dtype == ATX_F32 ? integral_typed<float, ATX_INTEGRAL_PRESSURE>(c, s) : integral_typed<double, ATX_INTEGRAL_PRESSURE>(c, s);
}
