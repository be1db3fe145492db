// Interpolation on a coordinate field: atx_coord_interpolate (include/atx_coord.h holds the statement), built into a library of its own,
// lib/libatx_coord.so — libatx's entry points are a fixed, tested set, as for the other companion libraries.
//
// The levels, heights and pltz kernels derive a point's coordinate column from sp and the A / B table; here it is a second stack in
// memory, strictly ascending or strictly descending PER POINT, and it has to be checked before it is searched.  ATX_COLUMNS, a 256-lane
// workgroup per tile of PT consecutive points, four phases:
//   1. stage     the tile's variable columns and its coordinate columns are two runs of PT x pitch elements: stage_columns
//                (atx_column_tile.hpp) copies each into LDS in order, each on its own route — 16 bytes per lane where column_route
//                allows (137 float64 levels at a tight pitch do not: 137 is odd; 13 float32 levels padded to a pitch of 16 do);
//   2. validate  one lane per (point, step): c[k+1] > c[k] keeps the point's "ascending" flag, c[k+1] < c[k] its "descending" flag;
//                a lane that clears a flag stores 0 — every writer stores the same value, so plain LDS stores combine them.  A NaN
//                clears both, an equal pair clears both, a turn clears one each.  The steps of a tile are consecutive LDS words: no
//                bank conflict, and every lane has work where a tile holds few points (29 points of 137 float32 levels).  One lane
//                per point walking its column was the alternative: at a pitch of 16 words its reads collide 16-fold, and at 137 levels
//                it leaves nine lanes in ten idle — chosen on those grounds, the two were not timed against each other;
//   3. bracket   one lane per (point, target): T once, the count #{k : e[k] <= T} by bisection in the LDS column — the column is
//                strictly monotone, so the count IS the upper bound, 8 LDS reads for 256 levels — read through (first, step) =
//                (0, +1) or (n - 1, -1), so a descending column is searched without being reversed and both directions run the same
//                instructions side by side; then w ONCE, in registers, and the lane walks the n_var variables in LDS and deposits
//                y into the tile's output run in LDS; one lane per point stores the point's bad byte;
//   4. store     the tile's output run leaves LDS in order: 16 bytes per lane where out allows, single elements otherwise; a
//                point's n_var x n_tgt outputs are one contiguous run, the tile's runs follow each other at out_pitch.
// No lane walks a column in HBM.  PT is what fits the LDS budget of the launch (tile_points over CoordCarve).
// ATX_FIELDS: one lane per (point, target), the 64 points of a wave consecutive: ONE strided walk of the coordinate rows gives both
// flags and the count (a count over a set does not ask for its order), two more loads give e[a], e[b], then 2 x n_var loads and n_var
// coalesced stores.  Both layouts and all routes evaluate the same float64 statements in the same order: same bits.
// No scratch (profiles/coord_resources.json).
#include "../../../include/atx_coord.h"
#include "../atx_column_tile.hpp"

namespace atx {

constexpr int kCoordMaxLevels = ATX_COORD_MAX_LEVELS;

// The bracket of a (point, target) pair as ROWS of the column in memory: a < 0: NaN;  a == b: a copy of row a;  else x[a] + w (x[b] - x[a]).
struct CoordBracket {
    int a, b;
    double w;
};

// The statement of include/atx_coord.h after the count, for a usable column of n rows read through e(j), j in ascending order of c:
// row j of that order is row first + step * j in memory.
template <typename E>
__device__ __forceinline__ CoordBracket coord_bracket(int count, int n, double T, int first, int step, int outside, E&& e) {
    CoordBracket r;
    r.a = r.b = -1;
    r.w = 0.0;
    if (count > 0 && count < n) {
        const double ea = e(count - 1), eb = e(count);
        const double num = T - ea, den = eb - ea;
        r.w = num / den;  // IEEE division
        r.a = first + step * (count - 1);
        r.b = first + step * count;
    } else if (count == n) {
        if (T == e(n - 1) || outside == ATX_COORD_NEAREST) r.a = r.b = first + step * (n - 1);
    } else if (outside == ATX_COORD_NEAREST) {
        r.a = r.b = first;
    }
    return r;
}

template <typename T>
__device__ __forceinline__ T coord_apply(const CoordBracket& r, T xa, T xb) {
    if (r.a < 0) return quiet_nan<T>();
    if (r.a == r.b) return xa;
    const double a = (double)xa, b = (double)xb;
    const double d = b - a;
    const double s = r.w * d;  // (-ffp-contract=off: a multiply and an add)
    return (T)(a + s);
}

// T of the statement: the rounded sum, or the target itself without an offset (-0.0 + 0.0 would be +0.0).
template <typename T>
__device__ __forceinline__ double coord_target(const double* __restrict__ targets, const T* __restrict__ offset, int t, int64_t p) {
    const double g = targets[t];
    if (offset == nullptr) return g;
    return g + (double)offset[p];
}

// Where the LDS of a tile of `pt` points holds what (byte offsets, multiples of 16): one definition for the launch and the kernel.
struct CoordCarve {
    int64_t cs, ys, up, down, total;  // (the staged variable columns start at 0)
};
__host__ __device__ inline CoordCarve coord_carve(int64_t pt, int x_pitch, int c_pitch, int elem, int per_point) {
    CoordCarve c;
    c.cs = round16(pt * x_pitch * elem);             // T [pt][c_pitch]
    c.ys = c.cs + round16(pt * c_pitch * elem);       // T [pt][per_point]
    c.up = c.ys + round16(pt * per_point * elem);     // int [pt]
    c.down = c.up + round16(pt * 4);                  // int [pt]
    c.total = c.down + round16(pt * 4);
    return c;
}

// ---- ATX_COLUMNS ---------------------------------------------------------------------------------------------------------------------
// VX, VC: elements per load when the variable and the coordinate columns are staged (Vec16<T>::N, or 1 for an odd pitch or an unaligned
// base); VO: elements per store of the output run; x_pitch, c_pitch: elements between the columns of two points in LDS (column_route).
template <typename T, int VX, int VC, int VO>
__global__ void __launch_bounds__(kTileBlock)
coord_columns_kernel(const T* __restrict__ src, const T* __restrict__ coord, T* __restrict__ out, const T* __restrict__ offset,
                     const T* __restrict__ floor, uint8_t* __restrict__ bad, const double* __restrict__ targets, int64_t n_pts, int n_var, int n_lev,
                     int n_tgt, int64_t src_pitch, int64_t coord_pitch, int64_t out_pitch, int PT, int x_pitch, int c_pitch, int outside) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int per_point = n_var * n_tgt;
    const CoordCarve lds = coord_carve(PT, x_pitch, c_pitch, (int)sizeof(T), per_point);
    T* xs = reinterpret_cast<T*>(smem);
    T* cs = reinterpret_cast<T*>(smem + lds.cs);
    T* ys = reinterpret_cast<T*>(smem + lds.ys);
    int* up = reinterpret_cast<int*>(smem + lds.up);      // 1: no step of the point's column fails c[k+1] > c[k]
    int* down = reinterpret_cast<int*>(smem + lds.down);  // 1: no step fails c[k+1] < c[k]

    const int tid = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * PT;
    const int npt = (int)(n_pts - p0 < PT ? n_pts - p0 : PT);

    // 1. stage
    stage_columns<T, VX>(src, xs, p0, npt, src_pitch, x_pitch, tid);
    stage_columns<T, VC>(coord, cs, p0, npt, coord_pitch, c_pitch, tid);
    for (int pt = tid; pt < npt; pt += kTileBlock) {
        up[pt] = 1;
        down[pt] = n_lev > 1 ? 1 : 0;
    }
    __syncthreads();
    // 2. validate
    if (n_lev > 1) {
        const int steps = n_lev - 1;
        TileWalk w(tid, steps);
        for (int i = tid; i < npt * steps; i += kTileBlock, w.next()) {
            const T* c = cs + (int64_t)w.row * c_pitch + w.col;
            const double here = (double)c[0], next = (double)c[1];
            if (!(next > here)) up[w.row] = 0;  // (a NaN fails both; every lane that writes, writes 0)
            if (!(next < here)) down[w.row] = 0;
        }
    } else {
        for (int pt = tid; pt < npt; pt += kTileBlock) {
            const T c0 = cs[(int64_t)pt * c_pitch];
            if (c0 != c0) up[pt] = 0;
        }
    }
    __syncthreads();
    // 3. bracket and apply
    {
        TileWalk w(tid, n_tgt);
        for (int i = tid; i < npt * n_tgt; i += kTileBlock, w.next()) {
            const int pt = w.row, t = w.col;
            const int ascending = up[pt], usable = ascending | down[pt];
            const int first = ascending ? 0 : n_lev - 1, step = ascending ? 1 : -1;
            const T* col = cs + (int64_t)pt * c_pitch;
            auto e = [&](int j) { return (double)col[first + step * j]; };
            const double Tg = coord_target<T>(targets, offset, t, p0 + pt);
            int count = 0, hi = n_lev;  // #{j : e(j) <= Tg} of a strictly ascending e: the first j with e(j) > Tg (a NaN target: 0)
            while (count < hi) {
                const int mid = (count + hi) >> 1;
                if (e(mid) <= Tg)
                    count = mid + 1;
                else
                    hi = mid;
            }
            CoordBracket r = coord_bracket(count, n_lev, Tg, first, step, outside, e);
            if (floor != nullptr && Tg < (double)floor[p0 + pt]) r.a = -1;
            if (!usable) r.a = -1;
            const int ra = r.a < 0 ? 0 : r.a, rb = r.b < 0 ? 0 : r.b;
            const T* x = xs + (int64_t)pt * x_pitch;
            T* y = ys + (int64_t)pt * per_point + t;
            for (int v = 0; v < n_var; ++v, x += n_lev, y += n_tgt) *y = coord_apply<T>(r, x[ra], x[rb]);
        }
    }
    if (bad != nullptr)
        for (int pt = tid; pt < npt; pt += kTileBlock) bad[p0 + pt] = (up[pt] | down[pt]) ? 0 : 1;
    __syncthreads();
    // 4. store (VO > 1: per_point and out_pitch are multiples of VO and out is 16-byte aligned)
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
template <typename T>
__global__ void __launch_bounds__(kTileBlock)
coord_fields_kernel(const T* __restrict__ src, const T* __restrict__ coord, T* __restrict__ out, const T* __restrict__ offset,
                    const T* __restrict__ floor, uint8_t* __restrict__ bad, const double* __restrict__ targets, int64_t n_pts, int n_var, int n_lev,
                    int n_tgt, int64_t src_pitch, int64_t coord_pitch, int64_t out_pitch, int outside) {
    const int64_t p = (int64_t)blockIdx.x * kTileBlock + threadIdx.x;
    if (p >= n_pts) return;
    const int t = blockIdx.y;
    const double Tg = coord_target<T>(targets, offset, t, p);
    // one walk: both flags and the count, which is the same over the column in either order
    double here = (double)coord[p];
    int up = here == here ? 1 : 0, down = n_lev > 1 ? 1 : 0, count = here <= Tg ? 1 : 0;
    for (int k = 1; k < n_lev; ++k) {
        const double next = (double)coord[(int64_t)k * coord_pitch + p];
        if (!(next > here)) up = 0;
        if (!(next < here)) down = 0;
        count += next <= Tg ? 1 : 0;
        here = next;
    }
    const int usable = up | down;
    const int first = up ? 0 : n_lev - 1, step = up ? 1 : -1;
    // (the rows read below stay inside the column whatever the count and the flags of a column that is not monotone)
    CoordBracket r = coord_bracket(count, n_lev, Tg, first, step, outside, [&](int j) { return (double)coord[(int64_t)(first + step * j) * coord_pitch + p]; });
    if (floor != nullptr && Tg < (double)floor[p]) r.a = -1;
    if (!usable) r.a = -1;
    if (bad != nullptr && t == 0) bad[p] = usable ? 0 : 1;
    const int ra = r.a < 0 ? 0 : r.a, rb = r.b < 0 ? 0 : r.b;
    for (int v = 0; v < n_var; ++v) {
        const T xa = src[((int64_t)v * n_lev + ra) * src_pitch + p], xb = src[((int64_t)v * n_lev + rb) * src_pitch + p];
        out[((int64_t)v * n_tgt + t) * out_pitch + p] = coord_apply<T>(r, xa, xb);
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
struct CoordCall {
    const void *src, *coord, *offset, *floor;
    void* out;
    uint8_t* bad;
    const double* targets;
    int64_t n_pts, src_pitch, coord_pitch, out_pitch;
    int n_var, n_lev, n_tgt, layout, outside;
};

template <typename T>
static int coord_typed(const CoordCall& c, hipStream_t st) {
    const char* fn = "atx_coord_interpolate";
    const T* src = static_cast<const T*>(c.src);
    const T* coord = static_cast<const T*>(c.coord);
    const T* offset = static_cast<const T*>(c.offset);
    const T* floor = static_cast<const T*>(c.floor);
    T* out = static_cast<T*>(c.out);
    if (c.layout == ATX_FIELDS) {
        const dim3 grid((unsigned)((c.n_pts + kTileBlock - 1) / kTileBlock), (unsigned)c.n_tgt);
        hipLaunchKernelGGL((coord_fields_kernel<T>), grid, dim3(kTileBlock), 0, st, src, coord, out, offset, floor, c.bad, c.targets, c.n_pts, c.n_var,
                           c.n_lev, c.n_tgt, c.src_pitch, c.coord_pitch, c.out_pitch, c.outside);
        ATX_LAUNCH_CHECK("coord_fields");
        return ATX_OK;
    }
    constexpr int VEC = Vec16<T>::N;
    const int rows = c.n_var * c.n_lev, per_point = c.n_var * c.n_tgt;
    const ColumnRoute xr = column_route<VEC>(c.src, c.src_pitch, rows), cr = column_route<VEC>(c.coord, c.coord_pitch, c.n_lev);
    const bool out_vector = aligned16(c.out) && c.out_pitch % VEC == 0 && per_point % VEC == 0;
    auto bytes = [&](int64_t pt) { return coord_carve(pt, xr.lds_pitch, cr.lds_pitch, (int)sizeof(T), per_point).total; };
    const int PT = tile_points(bytes);
    ATX_REQUIRE(PT > 0, ATX_ENOTIMPL, "%s: one point's %d rows, %d levels and %d outputs need %lld bytes of LDS, a workgroup has %lld (split the variables)",
                fn, rows, c.n_lev, per_point, (long long)bytes(1), (long long)kTileLdsLimit);
    const int64_t tiles = (c.n_pts + PT - 1) / PT;
    const size_t lds = (size_t)bytes(PT);
    auto launch = [&](auto vx, auto vc, auto vo) {
        hipLaunchKernelGGL((coord_columns_kernel<T, decltype(vx)::value, decltype(vc)::value, decltype(vo)::value>), dim3((unsigned)tiles), dim3(kTileBlock),
                           lds, st, src, coord, out, offset, floor, c.bad, c.targets, c.n_pts, c.n_var, c.n_lev, c.n_tgt, c.src_pitch, c.coord_pitch,
                           c.out_pitch, PT, xr.lds_pitch, cr.lds_pitch, c.outside);
        return 0;
    };
    const std::integral_constant<int, VEC> wide{};
    const std::integral_constant<int, 1> one{};
    auto with_width = [&](bool vector, auto&& f) { return vector ? f(wide) : f(one); };
    with_width(xr.vector, [&](auto vx) { return with_width(cr.vector, [&](auto vc) { return with_width(out_vector, [&](auto vo) { return launch(vx, vc, vo); }); }); });
    ATX_LAUNCH_CHECK("coord_columns");
    return ATX_OK;
}

// The bytes [lo, hi) that `rows` rows of a stack touch; a per-point vector is one row of a field-major stack.
struct CoordExtent {
    uintptr_t lo, hi;
    bool overlaps(const CoordExtent& o) const { return lo < o.hi && o.lo < hi; }
};
static CoordExtent coord_extent(const void* base, int64_t n_pts, int64_t rows, int64_t pitch, int layout, int elem) {
    const int64_t elements = layout == ATX_COLUMNS ? (n_pts - 1) * pitch + rows : (rows - 1) * pitch + n_pts;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(base);
    return {lo, lo + (uintptr_t)elements * (uintptr_t)elem};
}

}  // namespace atx

using namespace atx;

extern "C" int atx_coord_version(void) { return ATX_COORD_VERSION; }

extern "C" const char* atx_coord_last_error(void) { return last_error().c_str(); }

extern "C" int atx_coord_interpolate(const void* src, const void* coord, void* out, const void* offset, const void* floor, uint8_t* bad,
                                     const double* targets, int64_t n_pts, int64_t n_var, int64_t n_lev, int64_t n_tgt, int64_t src_pitch,
                                     int64_t coord_pitch, int64_t out_pitch, int dtype, int layout, int outside, void* stream) {
    const char* fn = "atx_coord_interpolate";
    ATX_REQUIRE(dtype == ATX_F32 || dtype == ATX_F64, ATX_EINVAL, "%s: bad dtype %d", fn, dtype);
    ATX_REQUIRE(layout == ATX_COLUMNS || layout == ATX_FIELDS, ATX_EINVAL, "%s: bad layout %d", fn, layout);
    ATX_REQUIRE(outside == ATX_COORD_NEAREST || outside == ATX_COORD_MISSING, ATX_EINVAL, "%s: unknown outside policy %d", fn, outside);
    ATX_REQUIRE(n_pts >= 0 && n_var >= 1 && n_lev >= 1 && n_tgt >= 0, ATX_EINVAL, "%s: bad sizes n_pts=%lld n_var=%lld n_lev=%lld n_tgt=%lld", fn,
                (long long)n_pts, (long long)n_var, (long long)n_lev, (long long)n_tgt);
    ATX_REQUIRE(n_lev <= kCoordMaxLevels, ATX_ENOTIMPL, "%s: n_lev=%lld exceeds the %d levels of one call", fn, (long long)n_lev, kCoordMaxLevels);
    ATX_REQUIRE(n_pts <= INT32_MAX && n_var <= 65535 && n_tgt <= 65535 && n_var * n_lev <= 65535 && n_var * n_tgt <= 65535, ATX_ENOTIMPL,
                "%s: sizes exceed the indexing of one launch (n_pts=%lld n_var=%lld n_lev=%lld n_tgt=%lld)", fn, (long long)n_pts, (long long)n_var,
                (long long)n_lev, (long long)n_tgt);
    if (layout == ATX_COLUMNS) {
        ATX_REQUIRE(src_pitch >= n_var * n_lev && coord_pitch >= n_lev && out_pitch >= n_var * n_tgt, ATX_ESHAPE,
                    "%s: column pitch (%lld, %lld, %lld) < rows (%lld, %lld, %lld)", fn, (long long)src_pitch, (long long)coord_pitch, (long long)out_pitch,
                    (long long)(n_var * n_lev), (long long)n_lev, (long long)(n_var * n_tgt));
    } else {
        ATX_REQUIRE(src_pitch >= n_pts && coord_pitch >= n_pts && out_pitch >= n_pts, ATX_ESHAPE, "%s: field pitch (%lld, %lld, %lld) < points %lld", fn,
                    (long long)src_pitch, (long long)coord_pitch, (long long)out_pitch, (long long)n_pts);
    }
    ATX_REQUIRE((src && coord) || n_pts == 0, ATX_EINVAL, "%s: null src / coord pointer", fn);
    ATX_REQUIRE(targets || n_tgt == 0, ATX_EINVAL, "%s: null targets", fn);
    ATX_REQUIRE(out || n_pts == 0 || n_tgt == 0, ATX_EINVAL, "%s: null out pointer", fn);
    if (n_pts == 0 || n_tgt == 0) return ATX_OK;
    const int elem = dtype == ATX_F32 ? 4 : 8;
    struct Named {
        const char* name;
        CoordExtent extent;
        bool present;
    };
    const Named inputs[] = {{"src", coord_extent(src, n_pts, n_var * n_lev, src_pitch, layout, elem), true},
                            {"coord", coord_extent(coord, n_pts, n_lev, coord_pitch, layout, elem), true},
                            {"offset", coord_extent(offset, n_pts, 1, n_pts, ATX_FIELDS, elem), offset != nullptr},
                            {"floor", coord_extent(floor, n_pts, 1, n_pts, ATX_FIELDS, elem), floor != nullptr}};
    const Named outputs[] = {{"out", coord_extent(out, n_pts, n_var * n_tgt, out_pitch, layout, elem), true},
                             {"bad", coord_extent(bad, n_pts, 1, n_pts, ATX_FIELDS, 1), bad != nullptr}};
    for (const Named& o : outputs)
        for (const Named& i : inputs) ATX_REQUIRE(!(o.present && i.present && o.extent.overlaps(i.extent)), ATX_EINVAL, "%s: %s overlaps %s", fn, o.name, i.name);
    ATX_REQUIRE(!(outputs[1].present && outputs[0].extent.overlaps(outputs[1].extent)), ATX_EINVAL, "%s: bad overlaps out", fn);
    CoordCall c;
    c.src = src, c.coord = coord, c.offset = offset, c.floor = floor, c.out = out, c.bad = bad, c.targets = targets;
    c.n_pts = n_pts, c.src_pitch = src_pitch, c.coord_pitch = coord_pitch, c.out_pitch = out_pitch;
    c.n_var = (int)n_var, c.n_lev = (int)n_lev, c.n_tgt = (int)n_tgt, c.layout = layout, c.outside = outside;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dtype == ATX_F32 ? coord_typed<float>(c, s) : coord_typed<double>(c, s);
}
