// Model levels to pressure levels: atx_levels_interpolate (include/atx_levels.h holds the statement), built into a library of its own,
// lib/libatx_levels.so — libatx's entry points are a fixed, tested set, as for libatx_plan / _mesh / _text / _missing / _stat.
//
// The one other vertical kernel, atx_pressure_at_height_stack (atx_vertical.hip), gives every lane its own column: in ATX_COLUMNS each
// of its load instructions touches 64 lines, one per column, and it runs at a tenth of the HBM peak.  Here a column is never walked by
// a lane.  ATX_COLUMNS, a 256-lane workgroup per tile of PT consecutive points, four phases:
//   1. stage     the tile's columns are one run of PT x src_pitch elements: stage_columns (atx_column_tile.hpp) copies it into LDS
//                in order, 16 bytes per lane where the stack allows (a wave's load covers 1 KiB of consecutive addresses), single
//                elements otherwise (256 B); the four coefficients of every row (A, B at m[k], m[k] + 1): to LDS once per workgroup;
//   2. pressures one lane per (point, level): p_full into LDS, float64 — and the level below it once more, to learn whether the
//                point's p_full never decreases; one lane per point: p_ground and sp;
//   3. brackets  one lane per (point, target): the count over the point's p_full — where it never decreases (and so holds no NaN) the
//                count over the whole column IS the upper bound a bisection finds, 8 LDS reads for 137 levels; any other column is
//                counted level by level, as the statement is written — then the bracket and the weight, ONCE per pair, kept in LDS
//                for all n_var variables;
//   4. apply     one lane per element of the tile's output, in output order: two LDS reads, y = x[a] + w (x[b] - x[a]), one store; a
//                point's n_var x n_tgt outputs are one contiguous run, the tile's runs follow each other at out_pitch.
// PT is what fits the LDS budget of the launch (tile_points over LevelsCarve).  ATX_FIELDS: one lane per (point, target), the 64 points of a wave
// consecutive: p_full is recomputed level by level from A, B (uniform) and sp, then 2 x n_var loads that coalesce where neighbouring
// points share a bracket, and n_var coalesced stores.  Both layouts evaluate the same float64 statements in the same order: same bits.
// The level map m[k] travels by value in the kernel arguments (ATX_LEVELS_MAX_LEVELS 16-bit entries): the host has checked it.
// No scratch (profiles/levels_resources.json).
#include "../../../include/atx_levels.h"
#include "../atx_column_tile.hpp"

namespace atx {

constexpr int kLevMaxLevels = ATX_LEVELS_MAX_LEVELS;

struct LevelMap {
    uint16_t m[kLevMaxLevels];  // m[k]: the 0-based model level of row k
};

struct Bracket {
    int a, b;  // a < 0: NaN;  a == b: a copy of row a;  else the interior of (a, b)
    double w;
};

template <bool LOG>
__device__ __forceinline__ double coordinate(double p) {
    if constexpr (LOG) return atx_log(p);
    return p;
}

// The statement of include/atx_levels.h after the count: `pfull(k)` gives p_full[k] of the point.
template <bool LOG, typename F>
__device__ __forceinline__ Bracket make_bracket(int count, int n, double P, double sp, double p_ground, int outside, F&& pfull) {
    Bracket r;
    r.a = r.b = -1;
    r.w = 0.0;
    if (sp != sp) return r;
    if (count > 0 && count < n) {
        r.a = count - 1;
        r.b = count;
        const double ca = coordinate<LOG>(pfull(r.a)), cb = coordinate<LOG>(pfull(r.b)), cp = coordinate<LOG>(P);
        r.w = (cp - ca) / (cb - ca);  // IEEE division
    } else if (count == n) {
        if (P <= p_ground || outside == ATX_LEVELS_NEAREST) r.a = r.b = n - 1;
    } else if (outside == ATX_LEVELS_NEAREST) {
        r.a = r.b = 0;
    }
    return r;
}

template <typename T>
__device__ __forceinline__ T interpolate(const Bracket& r, T xa, T xb) {
    if (r.a < 0) return quiet_nan<T>();
    if (r.a == r.b) return xa;
    const double a = (double)xa, b = (double)xb;
    const double d = b - a;
    const double s = r.w * d;  // (-ffp-contract=off: a multiply and an add)
    return (T)(a + s);
}

// Where the LDS of a tile of `pt` points holds what (byte offsets, multiples of 16): one definition for the launch and the kernel.
struct LevelsCarve {
    int64_t pf, sps, pg, bw, ba, bb, mono, coef, total;  // (the staged columns start at 0)
};
__host__ __device__ inline LevelsCarve levels_carve(int64_t pt, int lds_pitch, int elem, int n_lev, int n_tgt) {
    LevelsCarve c;
    c.pf = round16(pt * lds_pitch * elem);        // double [pt][n_lev]
    c.sps = c.pf + round16(pt * n_lev * 8);        // double [pt]
    c.pg = c.sps + round16(pt * 8);                // double [pt]
    c.bw = c.pg + round16(pt * 8);                 // double [pt][n_tgt]
    c.ba = c.bw + round16(pt * n_tgt * 8);         // int [pt][n_tgt]
    c.bb = c.ba + round16(pt * n_tgt * 4);         // int [pt][n_tgt]
    c.mono = c.bb + round16(pt * n_tgt * 4);       // int [pt]
    c.coef = c.mono + round16(pt * 4);             // double [4][n_lev]
    c.total = c.coef + round16((int64_t)4 * n_lev * 8);
    return c;
}

// ---- ATX_COLUMNS ---------------------------------------------------------------------------------------------------------------------
// VEC: elements per load of the staging phase (Vec16<T>::N, or 1 for an odd pitch or an unaligned base); lds_pitch: elements between
// the columns of two points in LDS (a multiple of VEC that covers n_var * n_lev).
template <typename T, int VEC, bool LOG>
__global__ void __launch_bounds__(kTileBlock)
levels_columns_kernel(const T* __restrict__ src, T* __restrict__ out, const T* __restrict__ sp, const double* __restrict__ A,
                      const double* __restrict__ B, const double* __restrict__ targets, const LevelMap map, int64_t n_pts, int n_var, int n_lev,
                      int n_tgt, int n_half, int64_t src_pitch, int64_t out_pitch, int PT, int lds_pitch, int outside) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const LevelsCarve lds = levels_carve(PT, lds_pitch, (int)sizeof(T), n_lev, n_tgt);
    T* xs = reinterpret_cast<T*>(smem);
    double* pf = reinterpret_cast<double*>(smem + lds.pf);
    double* sps = reinterpret_cast<double*>(smem + lds.sps);
    double* pg = reinterpret_cast<double*>(smem + lds.pg);
    double* bw = reinterpret_cast<double*>(smem + lds.bw);
    int* ba = reinterpret_cast<int*>(smem + lds.ba);
    int* bb = reinterpret_cast<int*>(smem + lds.bb);
    int* mono = reinterpret_cast<int*>(smem + lds.mono);  // 1: the point's p_full never decreases
    double* cA0 = reinterpret_cast<double*>(smem + lds.coef);  // A[m[k]], A[m[k] + 1], B[m[k]], B[m[k] + 1]
    double* cA1 = cA0 + n_lev;
    double* cB0 = cA1 + n_lev;
    double* cB1 = cB0 + n_lev;

    const int tid = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * PT;
    const int npt = (int)(n_pts - p0 < PT ? n_pts - p0 : PT);

    // 1. stage
    stage_columns<T, VEC>(src, xs, p0, npt, src_pitch, lds_pitch, tid);
    for (int k = tid; k < n_lev; k += kTileBlock) {
        const int j = map.m[k];
        cA0[k] = A[j];
        cA1[k] = A[j + 1];
        cB0[k] = B[j];
        cB1[k] = B[j + 1];
    }
    for (int pt = tid; pt < npt; pt += kTileBlock) mono[pt] = 1;
    __syncthreads();
    // 2. pressures (full_level's statements on the staged coefficients)
    for (int i = tid; i < npt * n_lev; i += kTileBlock) {
        const int pt = i / n_lev, k = i - pt * n_lev;
        const double s = (double)sp[p0 + pt];
        const double lo = cA0[k] + cB0[k] * s, hi = cA1[k] + cB1[k] * s;
        const double here = (lo + hi) / 2.0;
        pf[i] = here;
        if (k + 1 < n_lev) {
            const double lo1 = cA0[k + 1] + cB0[k + 1] * s, hi1 = cA1[k + 1] + cB1[k + 1] * s;
            const double below = (lo1 + hi1) / 2.0;
            if (!(here <= below)) mono[pt] = 0;  // (a NaN fails too; every lane that writes, writes 0)
        }
    }
    for (int pt = tid; pt < npt; pt += kTileBlock) {
        const double s = (double)sp[p0 + pt];
        sps[pt] = s;
        pg[pt] = half_level(A, B, n_half - 1, s);
    }
    __syncthreads();
    // 3. brackets
    for (int i = tid; i < npt * n_tgt; i += kTileBlock) {
        const int pt = i / n_tgt, t = i - pt * n_tgt;
        const double P = targets[t];
        const double* col = pf + pt * n_lev;
        int count = 0;
        if (mono[pt]) {  // #{k : col[k] <= P} of a column that never decreases: the first k with col[k] > P (a NaN target: 0)
            int hi = n_lev;
            while (count < hi) {
                const int mid = (count + hi) >> 1;
                if (col[mid] <= P)
                    count = mid + 1;
                else
                    hi = mid;
            }
        } else {
            for (int k = 0; k < n_lev; ++k) count += col[k] <= P ? 1 : 0;
        }
        const Bracket r = make_bracket<LOG>(count, n_lev, P, sps[pt], pg[pt], outside, [&](int k) { return col[k]; });
        ba[i] = r.a;
        bb[i] = r.b;
        bw[i] = r.w;
    }
    __syncthreads();
    // 4. apply
    const int per_point = n_var * n_tgt;
    for (int i = tid; i < npt * per_point; i += kTileBlock) {
        const int pt = i / per_point, j = i - pt * per_point;
        const int v = j / n_tgt, t = j - v * n_tgt;
        Bracket r;
        r.a = ba[pt * n_tgt + t];
        r.b = bb[pt * n_tgt + t];
        r.w = bw[pt * n_tgt + t];
        const T* x = xs + (int64_t)pt * lds_pitch + v * n_lev;
        const T xa = x[r.a < 0 ? 0 : r.a], xb = x[r.b < 0 ? 0 : r.b];
        out[(p0 + pt) * out_pitch + j] = interpolate<T>(r, xa, xb);
    }
}

// ---- ATX_FIELDS ----------------------------------------------------------------------------------------------------------------------
template <typename T, bool LOG>
__global__ void __launch_bounds__(kTileBlock)
levels_fields_kernel(const T* __restrict__ src, T* __restrict__ out, const T* __restrict__ sp, const double* __restrict__ A,
                     const double* __restrict__ B, const double* __restrict__ targets, const LevelMap map, int64_t n_pts, int n_var, int n_lev,
                     int n_tgt, int n_half, int64_t src_pitch, int64_t out_pitch, int outside) {
    const int64_t p = (int64_t)blockIdx.x * kTileBlock + threadIdx.x;
    if (p >= n_pts) return;
    const int t = blockIdx.y;
    const double s = (double)sp[p];
    const double P = targets[t];
    int count = 0;
    for (int k = 0; k < n_lev; ++k) count += full_level(A, B, map.m[k], s) <= P ? 1 : 0;  // (k is uniform: scalar loads of m, A, B)
    const double p_ground = half_level(A, B, n_half - 1, s);
    const Bracket r = make_bracket<LOG>(count, n_lev, P, s, p_ground, outside, [&](int k) { return full_level(A, B, map.m[k], s); });
    const int a = r.a < 0 ? 0 : r.a, b = r.b < 0 ? 0 : r.b;
    for (int v = 0; v < n_var; ++v) {
        const T xa = src[((int64_t)v * n_lev + a) * src_pitch + p], xb = src[((int64_t)v * n_lev + b) * src_pitch + p];
        out[((int64_t)v * n_tgt + t) * out_pitch + p] = interpolate<T>(r, xa, xb);
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
template <typename T>
static int levels_typed(const void* src_, void* out_, const void* sp_, const double* A, const double* B, const LevelMap& map, const double* targets,
                        int64_t n_pts, int n_var, int n_lev, int n_tgt, int n_half, int64_t sp, int64_t op, int layout, int coordinate, int outside,
                        hipStream_t st) {
    const char* fn = "atx_levels_interpolate";
    const T* src = static_cast<const T*>(src_);
    T* out = static_cast<T*>(out_);
    const T* sfc = static_cast<const T*>(sp_);
    const bool log = coordinate == ATX_LEVELS_LOG;
    if (layout == ATX_FIELDS) {
        const dim3 grid((unsigned)((n_pts + kTileBlock - 1) / kTileBlock), (unsigned)n_tgt);
        with_flag(log, [&](auto flag) {
            hipLaunchKernelGGL((levels_fields_kernel<T, decltype(flag)::value>), grid, dim3(kTileBlock), 0, st, src, out, sfc, A, B, targets, map, n_pts,
                               n_var, n_lev, n_tgt, n_half, sp, op, outside);
            return 0;
        });
        ATX_LAUNCH_CHECK("levels_fields");
        return ATX_OK;
    }
    constexpr int VEC = Vec16<T>::N;
    const int rows = n_var * n_lev;
    const ColumnRoute route = column_route<VEC>(src_, sp, rows);
    auto bytes = [&](int64_t pt) { return levels_carve(pt, route.lds_pitch, (int)sizeof(T), n_lev, n_tgt).total; };
    const int PT = tile_points(bytes);
    ATX_REQUIRE(PT > 0, ATX_ENOTIMPL, "%s: one point's %d rows, %d levels and %d targets need %lld bytes of LDS, a workgroup has %lld (split the variables)",
                fn, rows, n_lev, n_tgt, (long long)bytes(1), (long long)kTileLdsLimit);
    const int64_t tiles = (n_pts + PT - 1) / PT;
    const size_t lds = (size_t)bytes(PT);
    auto launch = [&](auto vec, auto flag) {
        hipLaunchKernelGGL((levels_columns_kernel<T, decltype(vec)::value, decltype(flag)::value>), dim3((unsigned)tiles), dim3(kTileBlock), lds, st, src, out,
                           sfc, A, B, targets, map, n_pts, n_var, n_lev, n_tgt, n_half, sp, op, PT, route.lds_pitch, outside);
        return 0;
    };
    with_flag(log, [&](auto flag) { return route.vector ? launch(std::integral_constant<int, VEC>{}, flag) : launch(std::integral_constant<int, 1>{}, flag); });
    ATX_LAUNCH_CHECK("levels_columns");
    return ATX_OK;
}

}  // namespace atx

using namespace atx;

extern "C" int atx_levels_version(void) { return ATX_LEVELS_VERSION; }

extern "C" const char* atx_levels_last_error(void) { return last_error().c_str(); }

extern "C" int atx_levels_interpolate(const void* src, void* out, const void* sp, const double* A, const double* B, const int32_t* level_index,
                                      const double* targets, int64_t n_pts, int64_t n_var, int64_t n_lev, int64_t n_tgt, int64_t n_half,
                                      int64_t src_pitch, int64_t out_pitch, int dtype, int layout, int coordinate, int outside, void* stream) {
    const char* fn = "atx_levels_interpolate";
    ATX_REQUIRE(dtype == ATX_F32 || dtype == ATX_F64, ATX_EINVAL, "%s: bad dtype %d", fn, dtype);
    ATX_REQUIRE(layout == ATX_COLUMNS || layout == ATX_FIELDS, ATX_EINVAL, "%s: bad layout %d", fn, layout);
    ATX_REQUIRE(coordinate == ATX_LEVELS_LINEAR || coordinate == ATX_LEVELS_LOG, ATX_EINVAL, "%s: unknown coordinate %d", fn, coordinate);
    ATX_REQUIRE(outside == ATX_LEVELS_NEAREST || outside == ATX_LEVELS_MISSING, ATX_EINVAL, "%s: unknown outside policy %d", fn, outside);
    ATX_REQUIRE(n_pts >= 0 && n_var >= 1 && n_lev >= 1 && n_tgt >= 0, ATX_EINVAL, "%s: bad sizes n_pts=%lld n_var=%lld n_lev=%lld n_tgt=%lld", fn,
                (long long)n_pts, (long long)n_var, (long long)n_lev, (long long)n_tgt);
    ATX_REQUIRE(n_half >= 2, ATX_EINVAL, "%s: n_half=%lld: a model has at least one level, two half levels", fn, (long long)n_half);
    ATX_REQUIRE(n_lev <= kLevMaxLevels, ATX_ENOTIMPL, "%s: n_lev=%lld exceeds the %d levels of one call", fn, (long long)n_lev, kLevMaxLevels);
    ATX_REQUIRE(n_pts <= INT32_MAX && n_var <= 65535 && n_tgt <= 65535 && n_half <= 65535 && n_var * n_lev <= 65535 && n_var * n_tgt <= 65535, ATX_ENOTIMPL,
                "%s: sizes exceed the indexing of one launch (n_pts=%lld n_var=%lld n_lev=%lld n_tgt=%lld n_half=%lld)", fn, (long long)n_pts,
                (long long)n_var, (long long)n_lev, (long long)n_tgt, (long long)n_half);
    if (layout == ATX_COLUMNS) {
        ATX_REQUIRE(src_pitch >= n_var * n_lev && out_pitch >= n_var * n_tgt, ATX_ESHAPE, "%s: column pitch (%lld, %lld) < rows (%lld, %lld)", fn,
                    (long long)src_pitch, (long long)out_pitch, (long long)(n_var * n_lev), (long long)(n_var * n_tgt));
    } else {
        ATX_REQUIRE(src_pitch >= n_pts && out_pitch >= n_pts, ATX_ESHAPE, "%s: field pitch (%lld, %lld) < points %lld", fn, (long long)src_pitch,
                    (long long)out_pitch, (long long)n_pts);
    }
    LevelMap map;
    memset(&map, 0, sizeof map);
    if (level_index) {
        for (int64_t k = 0; k < n_lev; ++k) {
            const int64_t m = level_index[k];
            ATX_REQUIRE(m >= 0 && m <= n_half - 2 && (k == 0 || m > level_index[k - 1]), ATX_EINVAL,
                        "%s: level_index[%lld] = %lld is not strictly increasing inside 0 .. %lld", fn, (long long)k, (long long)m, (long long)(n_half - 2));
            map.m[k] = (uint16_t)m;
        }
    } else {
        ATX_REQUIRE(n_lev <= n_half - 1, ATX_EINVAL, "%s: n_lev=%lld rows without a level_index need n_half >= %lld, got %lld", fn, (long long)n_lev,
                    (long long)(n_lev + 1), (long long)n_half);
        for (int64_t k = 0; k < n_lev; ++k) map.m[k] = (uint16_t)k;
    }
    ATX_REQUIRE(A && B, ATX_EINVAL, "%s: null A / B coefficients", fn);
    ATX_REQUIRE((src && sp) || n_pts == 0, ATX_EINVAL, "%s: null src / sp pointer", fn);
    ATX_REQUIRE(targets || n_tgt == 0, ATX_EINVAL, "%s: null targets", fn);
    ATX_REQUIRE(out || n_pts == 0 || n_tgt == 0, ATX_EINVAL, "%s: null out pointer", fn);
    if (n_pts == 0 || n_tgt == 0) return ATX_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == ATX_F32)
        return levels_typed<float>(src, out, sp, A, B, map, targets, n_pts, (int)n_var, (int)n_lev, (int)n_tgt, (int)n_half, src_pitch, out_pitch, layout,
                                   coordinate, outside, s);
    return levels_typed<double>(src, out, sp, A, B, map, targets, n_pts, (int)n_var, (int)n_lev, (int)n_tgt, (int)n_half, src_pitch, out_pitch, layout,
                                coordinate, outside, s);
}
