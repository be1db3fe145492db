// Geopotential on model levels: atx_geopotential_on_model_levels (include/atx_geopotential.h holds the statement), built into a library
// of its own, lib/libatx_geopotential.so — the entry points and the kernels of libatx_levels are a fixed, tested set, as libatx's are.
// The hydrostatic integral from the ground: z[k] = zs + (the delta R T of every layer below) + alpha R T of the level's own half
// layer — a sequential sum per column, with one logarithm and two divisions per (point, level).
//
// The other hydrostatic kernel, atx_pressure_at_height_stack (atx_vertical.hip), reduces a column to one pressure and gives every lane its
// own column in global memory.  Here, as in atx_levels.hip, no lane walks a column in HBM.  ATX_COLUMNS, a 256-lane workgroup per tile
// of PT consecutive points, four phases:
//   1. stage   the tile's t columns are one run of PT x t_pitch elements, its q columns one of PT x q_pitch: stage_columns copies each
//              into LDS in order, 16 bytes per lane where that stack allows (decided per stack), single elements otherwise; A and B of
//              the n_lev + 1 half levels the rows touch go to LDS once per workgroup; one lane per point: sp and zs, float64;
//   2. terms   one lane per (point, level): p_up, p_dn, r, delta = log(p_dn / p_up), alpha — the logarithm and the two divisions sit
//              here, 256 lanes wide — and the two products the sum needs, (alpha r) t and (delta r) t, into LDS.  A float64 stack's
//              terms take the places of the t and q they were made of (the lane that read them writes them); a float32 stack's go to
//              two float64 arrays of their own, with an odd pitch;
//   3. sum     one lane per point, from the ground up, over LDS: S[k], the sum of d over the levels below k, replaces d[k].  The one
//              sequential chain of the statement is these adds and nothing else; the reads do not depend on S, so kGeoBatch of them are
//              in flight ahead of the adds (the first version read, added and wrote level by level, a[k] too: 9.5 ms for O1280 x 137
//              float32, against 2.7 ms of the field-major kernel — profiles/geopotential_bench.json has the figures of this one);
//   4. store   one lane per element of the tile's output, in output order: z = zs + (S[k] + a[k]), rounded once; a point's n_lev values
//              are one contiguous run.
// PT is what fits the LDS budget of the launch (tile_points over GeoCarve).  ATX_FIELDS: one lane per point, bottom-up; every level is a
// coalesced load of t, one of q and a coalesced store; A and B are uniform.  Both layouts and both load routes evaluate the same
// float64 statements in the same order: same bits.  No scratch (profiles/geopotential_resources.json).
#include "../../../include/atx_geopotential.h"
#include "../atx_column_tile.hpp"

namespace atx {

constexpr int kGeoMaxLevels = ATX_GEOPOTENTIAL_MAX_LEVELS;
constexpr int kGeoBatch = 8;                        // LDS reads of the sum phase in flight ahead of the dependent adds
constexpr double kGeoRd = 287.0597, kGeoRv = 461.5250;  // J / (kg K), as in atx_vertical.hip
constexpr double kGeoLn2 = 0.6931471805599453;      // alpha of the IFS top level

// The two terms of one (point, level), the statement of include/atx_geopotential.h: `a` = (alpha r) t, `d` = (delta r) t (0.0 and unused at j == 0).
struct GeoTerms {
    double a, d;
};
__device__ __forceinline__ GeoTerms geo_terms(int j, double p_up, double p_dn, double t, double q) {
    const double om = 1.0 - q;
    const double dry = kGeoRd * om, wet = kGeoRv * q;
    const double r = dry + wet;
    GeoTerms g;
    if (j == 0) {
        g.a = (kGeoLn2 * r) * t;
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

// Where the LDS of a tile of `pt` points holds what (byte offsets, multiples of 16): one definition for the launch and the kernel.
// The staged t columns start at 0.  INPLACE (float64): the terms live in the staged columns, ta == 0 and td == q.
struct GeoCarve {
    int64_t q, ta, td, sps, zss, coef, total;
    int pa, pd;  // elements between two points' terms
};
__host__ __device__ inline GeoCarve geo_carve(int64_t pt, int lt, int lq, int elem, int n_lev) {
    GeoCarve c;
    c.q = round16(pt * lt * elem);                 // T [pt][lq]
    int64_t end = c.q + round16(pt * lq * elem);
    if (elem == 8) {
        c.ta = 0, c.td = c.q, c.pa = lt, c.pd = lq;
    } else {
        c.pa = c.pd = n_lev | 1;                   // odd: the points of the sum phase fall into different banks
        c.ta = end;                                // double [pt][pa]
        c.td = c.ta + round16(pt * c.pa * 8);      // double [pt][pd]
        end = c.td + round16(pt * c.pd * 8);
    }
    c.sps = end;                                   // double [pt]
    c.zss = c.sps + round16(pt * 8);               // double [pt]
    c.coef = c.zss + round16(pt * 8);              // double [2][n_lev + 1]
    c.total = c.coef + round16((int64_t)2 * (n_lev + 1) * 8);
    return c;
}

// ---- ATX_COLUMNS ---------------------------------------------------------------------------------------------------------------------
// VT, VQ: elements per load of the staging phase of t and of q (Vec16<T>::N, or 1 for an odd pitch or an unaligned base); lt, lq:
// elements between the columns of two points in LDS (a multiple of the stack's vector that covers n_lev).
template <typename T, int VT, int VQ>
__global__ void __launch_bounds__(kTileBlock)
geopotential_columns_kernel(const T* __restrict__ t, const T* __restrict__ q, const T* __restrict__ sp, const T* __restrict__ zs,
                            const double* __restrict__ A, const double* __restrict__ B, T* __restrict__ out, int64_t n_pts, int n_lev, int first,
                            int64_t t_pitch, int64_t q_pitch, int64_t out_pitch, int PT, int lt, int lq) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const GeoCarve lds = geo_carve(PT, lt, lq, (int)sizeof(T), n_lev);
    T* ts = reinterpret_cast<T*>(smem);
    T* qs = reinterpret_cast<T*>(smem + lds.q);
    double* ta = reinterpret_cast<double*>(smem + lds.ta);
    double* td = reinterpret_cast<double*>(smem + lds.td);
    double* sps = reinterpret_cast<double*>(smem + lds.sps);
    double* zss = reinterpret_cast<double*>(smem + lds.zss);
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
        zss[pt] = zs ? (double)zs[p0 + pt] : 0.0;
    }
    __syncthreads();
    // 2. terms
    TileWalk terms(tid, n_lev);
    for (int i = tid; i < npt * n_lev; i += kTileBlock, terms.next()) {
        const int pt = terms.row, k = terms.col;
        const double s = sps[pt];
        const double p_up = half_level(cA, cB, k, s), p_dn = half_level(cA, cB, k + 1, s);
        const double tk = (double)ts[pt * lt + k], qk = (double)qs[pt * lq + k];
        const GeoTerms g = geo_terms(first + k, p_up, p_dn, tk, qk);
        ta[pt * pa + k] = g.a;  // (float64: the places of tk and qk, which only this lane reads)
        td[pt * pd + k] = g.d;
    }
    __syncthreads();
    // 3. sum
    for (int pt = tid; pt < npt; pt += kTileBlock) {
        double* d = td + pt * pd;
        double S = 0.0;
        int k = n_lev - 1;
        for (; k >= kGeoBatch - 1; k -= kGeoBatch) {  // a batch of reads, then the dependent adds, then the writes
            double v[kGeoBatch];
#pragma unroll
            for (int i = 0; i < kGeoBatch; ++i) v[i] = d[k - i];
#pragma unroll
            for (int i = 0; i < kGeoBatch; ++i) {
                const double below = S;
                S = S + v[i];
                v[i] = below;
            }
#pragma unroll
            for (int i = 0; i < kGeoBatch; ++i) d[k - i] = v[i];
        }
        for (; k >= 0; --k) {
            const double below = S;
            S = S + d[k];  // (j == 0 adds 0.0 to a sum nothing reads again)
            d[k] = below;
        }
    }
    __syncthreads();
    // 4. store
    TileWalk store(tid, n_lev);
    for (int i = tid; i < npt * n_lev; i += kTileBlock, store.next()) {
        const int pt = store.row, k = store.col;
        const double lower = td[pt * pd + k] + ta[pt * pa + k];
        out[(p0 + pt) * out_pitch + k] = (T)(zss[pt] + lower);
    }
}

// ---- ATX_FIELDS ----------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(kTileBlock)
geopotential_fields_kernel(const T* __restrict__ t, const T* __restrict__ q, const T* __restrict__ sp, const T* __restrict__ zs,
                           const double* __restrict__ A, const double* __restrict__ B, T* __restrict__ out, int64_t n_pts, int n_lev, int first,
                           int64_t t_pitch, int64_t q_pitch, int64_t out_pitch) {
    const int64_t p = (int64_t)blockIdx.x * kTileBlock + threadIdx.x;
    if (p >= n_pts) return;
    const double s = (double)sp[p];
    const double z0 = zs ? (double)zs[p] : 0.0;
    double S = 0.0;
    for (int k = n_lev - 1; k >= 0; --k) {  // (k is uniform: scalar loads of A, B)
        const int j = first + k;
        const double p_up = half_level(A, B, j, s), p_dn = half_level(A, B, j + 1, s);
        const GeoTerms g = geo_terms(j, p_up, p_dn, (double)t[(int64_t)k * t_pitch + p], (double)q[(int64_t)k * q_pitch + p]);
        const double lower = S + g.a;
        out[(int64_t)k * out_pitch + p] = (T)(z0 + lower);
        S = S + g.d;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
template <typename T>
static int geopotential_typed(const void* t_, const void* q_, const void* sp_, const void* zs_, const double* A, const double* B, void* out_,
                              int64_t n_pts, int n_lev, int first, int64_t tp, int64_t qp, int64_t op, int layout, hipStream_t st) {
    const char* fn = "atx_geopotential_on_model_levels";
    const T* t = static_cast<const T*>(t_);
    const T* q = static_cast<const T*>(q_);
    const T* sp = static_cast<const T*>(sp_);
    const T* zs = static_cast<const T*>(zs_);
    T* out = static_cast<T*>(out_);
    if (layout == ATX_FIELDS) {
        const dim3 grid((unsigned)((n_pts + kTileBlock - 1) / kTileBlock));
        hipLaunchKernelGGL((geopotential_fields_kernel<T>), grid, dim3(kTileBlock), 0, st, t, q, sp, zs, A, B, out, n_pts, n_lev, first, tp, qp, op);
        ATX_LAUNCH_CHECK("geopotential_fields");
        return ATX_OK;
    }
    constexpr int VEC = Vec16<T>::N;
    const ColumnRoute rt = column_route<VEC>(t_, tp, n_lev), rq = column_route<VEC>(q_, qp, n_lev);
    const int lt = rt.lds_pitch, lq = rq.lds_pitch;
    auto bytes = [&](int64_t pt) { return geo_carve(pt, lt, lq, (int)sizeof(T), n_lev).total; };
    const int PT = tile_points(bytes);
    ATX_REQUIRE(PT > 0, ATX_ENOTIMPL, "%s: one point's %d levels need %lld bytes of LDS, a workgroup has %lld", fn, n_lev, (long long)bytes(1),
                (long long)kTileLdsLimit);
    const int64_t tiles = (n_pts + PT - 1) / PT;
    const size_t lds = (size_t)bytes(PT);
    with_flag(rt.vector, [&](auto vec_t) {
        return with_flag(rq.vector, [&](auto vec_q) {
            constexpr int VT = decltype(vec_t)::value ? VEC : 1, VQ = decltype(vec_q)::value ? VEC : 1;
            hipLaunchKernelGGL((geopotential_columns_kernel<T, VT, VQ>), dim3((unsigned)tiles), dim3(kTileBlock), lds, st, t, q, sp, zs, A, B, out,
                               n_pts, n_lev, first, tp, qp, op, PT, lt, lq);
            return 0;
        });
    });
    ATX_LAUNCH_CHECK("geopotential_columns");
    return ATX_OK;
}

// The bytes [lo, hi) a stack of the shape touches.
static void geo_extent(const void* base, int64_t n_pts, int64_t n_lev, int64_t pitch, int layout, int elem, uintptr_t& lo, uintptr_t& hi) {
    const int64_t elements = layout == ATX_COLUMNS ? (n_pts - 1) * pitch + n_lev : (n_lev - 1) * pitch + n_pts;
    lo = reinterpret_cast<uintptr_t>(base);
    hi = lo + (uintptr_t)elements * (uintptr_t)elem;
}

}  // namespace atx

using namespace atx;

extern "C" int atx_geopotential_version(void) { return ATX_GEOPOTENTIAL_VERSION; }

extern "C" const char* atx_geopotential_last_error(void) { return last_error().c_str(); }

extern "C" int atx_geopotential_on_model_levels(const void* t, const void* q, const void* sp, const void* zs, const double* A, const double* B, void* out,
                                       int64_t n_pts, int64_t n_lev, int64_t n_half, int64_t t_pitch, int64_t q_pitch, int64_t out_pitch, int dtype,
                                       int layout, void* stream) {
    const char* fn = "atx_geopotential_on_model_levels";
    ATX_REQUIRE(dtype == ATX_F32 || dtype == ATX_F64, ATX_EINVAL, "%s: bad dtype %d", fn, dtype);
    ATX_REQUIRE(layout == ATX_COLUMNS || layout == ATX_FIELDS, ATX_EINVAL, "%s: bad layout %d", fn, layout);
    ATX_REQUIRE(n_pts >= 0 && n_lev >= 1, ATX_EINVAL, "%s: bad sizes n_pts=%lld n_lev=%lld", fn, (long long)n_pts, (long long)n_lev);
    ATX_REQUIRE(n_half >= 2, ATX_EINVAL, "%s: n_half=%lld: a model has at least one level, two half levels", fn, (long long)n_half);
    ATX_REQUIRE(n_lev <= n_half - 1, ATX_EINVAL, "%s: n_lev=%lld rows are the lowest levels of a model of %lld, n_half=%lld", fn, (long long)n_lev,
                (long long)(n_half - 1), (long long)n_half);
    ATX_REQUIRE(n_lev <= kGeoMaxLevels, ATX_ENOTIMPL, "%s: n_lev=%lld exceeds the %d levels of one call", fn, (long long)n_lev, kGeoMaxLevels);
    ATX_REQUIRE(n_pts <= INT32_MAX && n_half <= 65535, ATX_ENOTIMPL, "%s: sizes exceed the indexing of one launch (n_pts=%lld n_half=%lld)", fn,
                (long long)n_pts, (long long)n_half);
    const int64_t least = layout == ATX_COLUMNS ? n_lev : n_pts;
    ATX_REQUIRE(t_pitch >= least && q_pitch >= least && out_pitch >= least, ATX_ESHAPE, "%s: %s pitch (%lld, %lld, %lld) < %s %lld", fn,
                layout == ATX_COLUMNS ? "column" : "field", (long long)t_pitch, (long long)q_pitch, (long long)out_pitch,
                layout == ATX_COLUMNS ? "rows" : "points", (long long)least);
    ATX_REQUIRE(A && B, ATX_EINVAL, "%s: null A / B coefficients", fn);
    ATX_REQUIRE((t && q && sp) || n_pts == 0, ATX_EINVAL, "%s: null t / q / sp pointer", fn);
    ATX_REQUIRE(out || n_pts == 0, ATX_EINVAL, "%s: null out pointer", fn);
    if (n_pts == 0) return ATX_OK;
    const int elem = dtype == ATX_F32 ? 4 : 8;
    uintptr_t olo, ohi, lo, hi;
    geo_extent(out, n_pts, n_lev, out_pitch, layout, elem, olo, ohi);
    geo_extent(t, n_pts, n_lev, t_pitch, layout, elem, lo, hi);
    ATX_REQUIRE(!(olo < hi && lo < ohi), ATX_EINVAL, "%s: out overlaps t", fn);
    geo_extent(q, n_pts, n_lev, q_pitch, layout, elem, lo, hi);
    ATX_REQUIRE(!(olo < hi && lo < ohi), ATX_EINVAL, "%s: out overlaps q", fn);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int first = (int)(n_half - 1 - n_lev);
    if (dtype == ATX_F32) return geopotential_typed<float>(t, q, sp, zs, A, B, out, n_pts, (int)n_lev, first, t_pitch, q_pitch, out_pitch, layout, s);
    return geopotential_typed<double>(t, q, sp, zs, A, B, out, n_pts, (int)n_lev, first, t_pitch, q_pitch, out_pitch, layout, s);
}
