// The column search: atx_search_columns (include/atx_search.h holds the statement), built into a library of its own,
// lib/libatx_search.so — libatx's entry points are a fixed, tested set, as for the other companion libraries.
//
// The coordinate kernel (coord/atx_coord.hip) checks that a column is monotone and bisects it.  Here nothing is monotone: the answer is
// the FIRST step in scan order that satisfies a predicate, or the first arg-extremum, and a bisection cannot find either.  What a lane
// is, is therefore different.  ATX_COLUMNS, a 256-lane workgroup per tile of PT consecutive points, four phases:
//   1. stage    the tile's variable columns and its search columns are two runs of PT x pitch elements: stage_columns
//               (atx_column_tile.hpp) copies each into LDS in order, each on its own route — 16 bytes per lane where column_route allows;
//               level_values, where given, are copied next to them;
//   2. search   WAVE-COOPERATIVE: lanes are the steps of a column, not points.  A wave takes a (point, target) pair; lane j evaluates
//               the predicate of memory step 64 c + j (rows m, m + 1) from LDS — consecutive words, no bank conflict — __ballot gives
//               the 64 predicates as one mask, its first set bit (FORWARD) or its last (BACKWARD) is the answer and __popcll its count.
//               256 levels are four ballots at most, taken in scan order, and the wave stops at the first mask that is not empty
//               unless the count is asked.  A column of W = 2^ceil(log2 n) <= 32 rows leaves lanes idle, so 64 / W pairs share a
//               wave: the ballot is cut into segments of W bits with a shift and a mask (13 pressure levels: four pairs a ballot, 37:
//               one).  An extremum is a reduction of (value, scan index) pairs over the W lanes of a segment by __shfl_xor, the
//               smaller scan index winning among equal values: "greater, or equal and earlier" is a total order on the pairs, so the
//               result does not depend on the shape of the reduction.  The first lane of a segment computes w ONCE and leaves
//               (a, b, w) in LDS and the count in memory;
//   3. apply    one lane per (point, variable, target): x[a] + w (x[b] - x[a]) from LDS into the tile's output run in LDS;
//   4. store    the tile's output run leaves LDS in order: 16 bytes per lane where out allows, single elements otherwise; a point's
//               outputs are one contiguous run, the tile's runs follow each other at out_pitch.
// No lane walks a column in HBM.  PT is what fits the LDS budget of the launch (tile_points over SearchCarve).
// ATX_FIELDS: one lane per (point, target), the 64 points of a wave consecutive: ONE strided walk of the search rows in scan order with
// the state in registers — the first hit is kept and the walk goes on only where the count is asked — then 2 x n_var loads and the
// coalesced stores.  Both layouts and all routes evaluate the same float64 statements in the same order: same bits.
// No scratch (profiles/search_resources.json).
#include "../../../include/atx_search.h"
#include "../atx_column_tile.hpp"

namespace atx {

constexpr int kSearchMaxLevels = ATX_SEARCH_MAX_LEVELS;
constexpr int kTileWaves = kTileBlock / kWave;

// The answer of a (point, target) pair as ROWS of the column in memory: a < 0: NaN;  a == b: a copy of row a;  else x[a] + w (x[b] - x[a]).
struct SearchHit {
    int a, b;
    double w;
};

__device__ __forceinline__ bool is_extremum(int mode) { return mode >= ATX_SEARCH_MAX; }

// Step (here -> next), both in SCAN order, against the target: one compare of each kind is strict (a NaN anywhere: false).
__device__ __forceinline__ bool search_crosses(int mode, double here, double next, double T) {
    const bool up = here <= T && T < next, down = here >= T && T > next;
    return mode == ATX_SEARCH_UP ? up : mode == ATX_SEARCH_DOWN ? down : (up || down);
}

// (v, k) is better than (bv, bk): nearer the extremum, or equal and earlier in the scan.  bk < 0: nothing yet.  v is not NaN.
__device__ __forceinline__ bool search_better(int mode, double v, int k, double bv, int bk) {
    if (bk < 0) return true;
    const bool beyond = mode == ATX_SEARCH_MAX ? v > bv : v < bv;
    return beyond || (v == bv && k < bk);
}

// The statement after the search.  crossing: the memory rows of the first step in scan order (a -> b), or a < 0 and `last`, the row
// the scan reads last, which is copied where it equals T.
template <typename E>
__device__ __forceinline__ SearchHit search_hit(int a, int b, int last, double T, E&& e) {
    SearchHit r;
    r.a = r.b = -1;
    r.w = 0.0;
    if (a >= 0) {
        const double ea = e(a), eb = e(b);
        const double num = T - ea, den = eb - ea;
        r.w = num / den;  // IEEE division
        r.a = a, r.b = b;
    } else if (e(last) == T) {
        r.a = r.b = last;
    }
    return r;
}

template <typename T>
__device__ __forceinline__ T search_apply(const SearchHit& r, T xa, T xb) {
    if (r.a < 0) return quiet_nan<T>();
    if (r.a == r.b) return xa;
    const double a = (double)xa, b = (double)xb;
    const double d = b - a;
    const double s = r.w * d;  // (-ffp-contract=off: a multiply and an add)
    return (T)(a + s);
}

// level_values as the last variable: float64 in, the stack's type out.
template <typename T>
__device__ __forceinline__ T search_apply_levels(const SearchHit& r, double la, double lb) {
    if (r.a < 0) return quiet_nan<T>();
    if (r.a == r.b) return (T)la;
    const double d = lb - la;
    const double s = r.w * d;
    return (T)(la + s);
}

__device__ __forceinline__ uint8_t saturate255(int n) { return (uint8_t)(n > 255 ? 255 : n); }

// Where the LDS of a tile of `pt` points holds what (byte offsets, multiples of 16): one definition for the launch and the kernel.
struct SearchCarve {
    int64_t ss, ys, lv, hw, hab, total;  // (the staged variable columns start at 0)
};
__host__ __device__ inline SearchCarve search_carve(int64_t pt, int x_pitch, int s_pitch, int elem, int per_point, int n_tgt, int n_lev, int has_lv) {
    SearchCarve c;
    c.ss = round16(pt * x_pitch * elem);                 // T [pt][s_pitch]
    c.ys = c.ss + round16(pt * s_pitch * elem);          // T [pt][per_point]
    c.lv = c.ys + round16(pt * per_point * elem);        // double [n_lev]
    c.hw = c.lv + (has_lv ? round16(n_lev * 8) : 0);     // double [pt][n_tgt]
    c.hab = c.hw + round16(pt * n_tgt * 8);              // int2 [pt][n_tgt]
    c.total = c.hab + round16(pt * n_tgt * 8);
    return c;
}

// The lanes of a segment: W = the least power of two >= n_lev, 64 at most.
static inline int search_segment(int n_lev) {
    int w = 1;
    while (w < n_lev && w < kWave) w *= 2;
    return w;
}

// ---- ATX_COLUMNS ---------------------------------------------------------------------------------------------------------------------
// VX, VS: elements per load when the variable and the search columns are staged (Vec16<T>::N, or 1 for an odd pitch or an unaligned
// base); VO: elements per store of the output run; x_pitch, s_pitch: elements between the columns of two points in LDS (column_route).
// W: the lanes of a segment (search_segment), log2W its logarithm.
template <typename T, int VX, int VS, int VO>
__global__ void __launch_bounds__(kTileBlock)
search_columns_kernel(const T* __restrict__ src, const T* __restrict__ search, T* __restrict__ out, uint8_t* __restrict__ count,
                      const double* __restrict__ targets, const double* __restrict__ level_values, int64_t n_pts, int n_var, int n_lev, int n_tgt,
                      int64_t src_pitch, int64_t search_pitch, int64_t out_pitch, int PT, int x_pitch, int s_pitch, int backward, int mode, int W,
                      int log2W) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int has_lv = level_values != nullptr ? 1 : 0;
    const int per_point = (n_var + has_lv) * n_tgt;
    const SearchCarve lds = search_carve(PT, x_pitch, s_pitch, (int)sizeof(T), per_point, n_tgt, n_lev, has_lv);
    T* xs = reinterpret_cast<T*>(smem);
    T* ss = reinterpret_cast<T*>(smem + lds.ss);
    T* ys = reinterpret_cast<T*>(smem + lds.ys);
    double* lv = reinterpret_cast<double*>(smem + lds.lv);
    double* hw = reinterpret_cast<double*>(smem + lds.hw);
    int2* hab = reinterpret_cast<int2*>(smem + lds.hab);

    const int tid = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * PT;
    const int npt = (int)(n_pts - p0 < PT ? n_pts - p0 : PT);

    // 1. stage
    if (n_var > 0) stage_columns<T, VX>(src, xs, p0, npt, src_pitch, x_pitch, tid);
    stage_columns<T, VS>(search, ss, p0, npt, search_pitch, s_pitch, tid);
    if (has_lv)
        for (int k = tid; k < n_lev; k += kTileBlock) lv[k] = level_values[k];
    __syncthreads();

    // 2. search: wave `wave` takes the groups wave, wave + 4, ... of G = 64 / W (point, target) pairs; every branch around a ballot or a
    //    shuffle is uniform over the wave
    {
        const int lane = tid & (kWave - 1), wave = tid >> 6;
        const int G = kWave >> log2W, g = lane >> log2W, j = lane & (W - 1);
        const unsigned long long segment = W == kWave ? ~0ull : ((1ull << W) - 1ull);
        const int pairs = npt * n_tgt, groups = (pairs + G - 1) / G;
        const bool extremum = is_extremum(mode);
        const int items = extremum ? n_lev : n_lev - 1;  // rows, or steps
        const int chunks = items > 0 ? (items + kWave - 1) / kWave : 0;
        const int last = backward ? 0 : n_lev - 1;  // the row the scan reads last
        for (int grp = wave; grp < groups; grp += kTileWaves) {
            const int pair = grp * G + g;
            const bool live = pair < pairs;
            const int pt = live ? pair / n_tgt : 0, t = live ? pair - pt * n_tgt : 0;
            const T* col = ss + (int64_t)pt * s_pitch;
            int a = -1, b = -1, n_found = 0;
            if (!extremum) {
                const double Tg = targets[t];
                for (int i = 0; i < chunks; ++i) {
                    const int c = backward ? chunks - 1 - i : i;  // the chunks in scan order
                    const int m = c * kWave + j;                   // memory step m: rows m, m + 1
                    bool hit = false;
                    if (live && m < items) {
                        const double lo = (double)col[m], hi = (double)col[m + 1];
                        hit = backward ? search_crosses(mode, hi, lo, Tg) : search_crosses(mode, lo, hi, Tg);
                    }
                    const unsigned long long mask = (__ballot(hit) >> (g << log2W)) & segment;
                    n_found += __popcll(mask);
                    if (a < 0 && mask != 0ull) {
                        const int first = c * kWave + (backward ? 63 - __clzll((long long)mask) : __ffsll((long long)mask) - 1);
                        a = backward ? first + 1 : first;
                        b = backward ? first : first + 1;
                    }
                    if (count == nullptr && G == 1 && a >= 0) break;  // (G == 1: `a` is uniform over the wave)
                }
                if (live && j == 0) {
                    const SearchHit r = search_hit(a, b, last, Tg, [&](int row) { return (double)col[row]; });
                    hw[pair] = r.w;
                    hab[pair] = make_int2(r.a, r.b);
                    if (count != nullptr) count[p0 * n_tgt + pair] = saturate255(n_found);
                }
            } else {
                // every lane's own best over its rows 64 c + j, then the segment's
                double bv = 0.0;
                int bk = -1;
                for (int c = 0; c < chunks; ++c) {
                    const int m = c * kWave + j;
                    if (live && m < items) {
                        const double v = (double)col[m];
                        const int k = backward ? n_lev - 1 - m : m;
                        if (v == v && search_better(mode, v, k, bv, bk)) bv = v, bk = k;
                    }
                }
                for (int offset = W >> 1; offset > 0; offset >>= 1) {
                    const double ov = __shfl_xor(bv, offset);
                    const int ok = __shfl_xor(bk, offset);
                    if (ok >= 0 && search_better(mode, ov, ok, bv, bk)) bv = ov, bk = ok;
                }
                if (count != nullptr) {
                    for (int c = 0; c < chunks; ++c) {
                        const int m = c * kWave + j;
                        const bool equal = live && m < items && bk >= 0 && (double)col[m] == bv;
                        n_found += __popcll((__ballot(equal) >> (g << log2W)) & segment);
                    }
                }
                if (live && j == 0) {
                    const int row = bk < 0 ? -1 : (backward ? n_lev - 1 - bk : bk);
                    hw[pair] = 0.0;
                    hab[pair] = make_int2(row, row);
                    if (count != nullptr) count[p0 + pair] = saturate255(n_found);
                }
            }
        }
    }
    __syncthreads();
    if (per_point == 0) return;
    // 3. apply: one lane per (point, variable, target)
    {
        TileWalk w(tid, per_point);
        for (int i = tid; i < npt * per_point; i += kTileBlock, w.next()) {
            const int pt = w.row, v = n_tgt == 1 ? w.col : w.col / n_tgt, t = w.col - v * n_tgt;
            const int2 ab = hab[pt * n_tgt + t];
            SearchHit r;
            r.a = ab.x, r.b = ab.y, r.w = hw[pt * n_tgt + t];
            const int ra = r.a < 0 ? 0 : r.a, rb = r.b < 0 ? 0 : r.b;
            T y;
            if (v < n_var) {
                const T* x = xs + (int64_t)pt * x_pitch + v * n_lev;
                y = search_apply<T>(r, x[ra], x[rb]);
            } else {
                y = search_apply_levels<T>(r, lv[ra], lv[rb]);
            }
            ys[(int64_t)pt * per_point + w.col] = y;
        }
    }
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
search_fields_kernel(const T* __restrict__ src, const T* __restrict__ search, T* __restrict__ out, uint8_t* __restrict__ count,
                     const double* __restrict__ targets, const double* __restrict__ level_values, int64_t n_pts, int n_var, int n_lev, int n_tgt,
                     int64_t src_pitch, int64_t search_pitch, int64_t out_pitch, int backward, int mode) {
    const int64_t p = (int64_t)blockIdx.x * kTileBlock + threadIdx.x;
    if (p >= n_pts) return;
    const int t = blockIdx.y;
    const int first = backward ? n_lev - 1 : 0, step = backward ? -1 : 1;
    auto e = [&](int row) { return (double)search[(int64_t)row * search_pitch + p]; };
    SearchHit r;
    int n_found = 0;
    if (!is_extremum(mode)) {
        const double Tg = targets[t];
        int a = -1, b = -1;
        double here = e(first);
        for (int k = 0; k + 1 < n_lev; ++k) {  // scan step k: rows first + step k -> first + step (k + 1)
            const int row = first + step * (k + 1);
            const double next = e(row);
            if (search_crosses(mode, here, next, Tg)) {
                ++n_found;
                if (a < 0) a = row - step, b = row;
                if (count == nullptr) break;
            }
            here = next;
        }
        r = search_hit(a, b, first + step * (n_lev - 1), Tg, e);
    } else {
        double bv = 0.0;
        int bk = -1;
        for (int k = 0; k < n_lev; ++k) {
            const double v = e(first + step * k);
            if (v == v) {
                if (search_better(mode, v, k, bv, bk))
                    bv = v, bk = k, n_found = 1;  // (k grows: better here means strictly beyond, or the first value)
                else if (v == bv)
                    ++n_found;
            }
        }
        r.a = r.b = bk < 0 ? -1 : first + step * bk;
        r.w = 0.0;
    }
    if (count != nullptr) count[(int64_t)t * n_pts + p] = saturate255(n_found);
    const int ra = r.a < 0 ? 0 : r.a, rb = r.b < 0 ? 0 : r.b;
    for (int v = 0; v < n_var; ++v) {
        const T xa = src[((int64_t)v * n_lev + ra) * src_pitch + p], xb = src[((int64_t)v * n_lev + rb) * src_pitch + p];
        out[((int64_t)v * n_tgt + t) * out_pitch + p] = search_apply<T>(r, xa, xb);
    }
    if (level_values != nullptr) out[((int64_t)n_var * n_tgt + t) * out_pitch + p] = search_apply_levels<T>(r, level_values[ra], level_values[rb]);
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
struct SearchCall {
    const void *src, *search;
    void* out;
    uint8_t* count;
    const double *targets, *level_values;
    int64_t n_pts, src_pitch, search_pitch, out_pitch;
    int n_var, n_lev, n_tgt, layout, backward, mode;
};

template <typename T>
static int search_typed(const SearchCall& c, hipStream_t st) {
    const char* fn = "atx_search_columns";
    const T* src = static_cast<const T*>(c.src);
    const T* search = static_cast<const T*>(c.search);
    T* out = static_cast<T*>(c.out);
    if (c.layout == ATX_FIELDS) {
        const dim3 grid((unsigned)((c.n_pts + kTileBlock - 1) / kTileBlock), (unsigned)c.n_tgt);
        hipLaunchKernelGGL((search_fields_kernel<T>), grid, dim3(kTileBlock), 0, st, src, search, out, c.count, c.targets, c.level_values, c.n_pts, c.n_var,
                           c.n_lev, c.n_tgt, c.src_pitch, c.search_pitch, c.out_pitch, c.backward, c.mode);
        ATX_LAUNCH_CHECK("search_fields");
        return ATX_OK;
    }
    constexpr int VEC = Vec16<T>::N;
    const int has_lv = c.level_values != nullptr ? 1 : 0;
    const int rows = c.n_var * c.n_lev, per_point = (c.n_var + has_lv) * c.n_tgt;
    const ColumnRoute none{false, 0};
    const ColumnRoute xr = rows > 0 ? column_route<VEC>(c.src, c.src_pitch, rows) : none, sr = column_route<VEC>(c.search, c.search_pitch, c.n_lev);
    const bool out_vector = per_point > 0 && aligned16(c.out) && c.out_pitch % VEC == 0 && per_point % VEC == 0;
    auto bytes = [&](int64_t pt) { return search_carve(pt, xr.lds_pitch, sr.lds_pitch, (int)sizeof(T), per_point, c.n_tgt, c.n_lev, has_lv).total; };
    const int PT = tile_points(bytes);
    ATX_REQUIRE(PT > 0, ATX_ENOTIMPL, "%s: one point's %d rows, %d levels and %d outputs need %lld bytes of LDS, a workgroup has %lld (split the variables)",
                fn, rows, c.n_lev, per_point, (long long)bytes(1), (long long)kTileLdsLimit);
    const int64_t tiles = (c.n_pts + PT - 1) / PT;
    const size_t lds = (size_t)bytes(PT);
    const int W = search_segment(c.n_lev);
    int log2W = 0;
    while ((1 << log2W) < W) ++log2W;
    auto launch = [&](auto vx, auto vs, auto vo) {
        hipLaunchKernelGGL((search_columns_kernel<T, decltype(vx)::value, decltype(vs)::value, decltype(vo)::value>), dim3((unsigned)tiles), dim3(kTileBlock),
                           lds, st, src, search, out, c.count, c.targets, c.level_values, c.n_pts, c.n_var, c.n_lev, c.n_tgt, c.src_pitch, c.search_pitch,
                           c.out_pitch, PT, xr.lds_pitch, sr.lds_pitch, c.backward, c.mode, W, log2W);
        return 0;
    };
    const std::integral_constant<int, VEC> wide{};
    const std::integral_constant<int, 1> one{};
    auto with_width = [&](bool vector, auto&& f) { return vector ? f(wide) : f(one); };
    with_width(xr.vector, [&](auto vx) { return with_width(sr.vector, [&](auto vs) { return with_width(out_vector, [&](auto vo) { return launch(vx, vs, vo); }); }); });
    ATX_LAUNCH_CHECK("search_columns");
    return ATX_OK;
}

// The bytes [lo, hi) that `rows` rows of a stack touch; a vector is one row of a field-major stack.
struct SearchExtent {
    uintptr_t lo, hi;
    bool overlaps(const SearchExtent& o) const { return lo < o.hi && o.lo < hi; }
};
static SearchExtent search_extent(const void* base, int64_t n_pts, int64_t rows, int64_t pitch, int layout, int elem) {
    const int64_t elements = layout == ATX_COLUMNS ? (n_pts - 1) * pitch + rows : (rows - 1) * pitch + n_pts;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(base);
    return {lo, lo + (uintptr_t)elements * (uintptr_t)elem};
}

}  // namespace atx

using namespace atx;

extern "C" int atx_search_version(void) { return ATX_SEARCH_VERSION; }

extern "C" const char* atx_search_last_error(void) { return last_error().c_str(); }

extern "C" int atx_search_columns(const void* src, const void* search, void* out, uint8_t* count, const double* targets, const double* level_values,
                                  int64_t n_pts, int64_t n_var, int64_t n_lev, int64_t n_tgt, int64_t src_pitch, int64_t search_pitch, int64_t out_pitch,
                                  int dtype, int layout, int direction, int mode, void* stream) {
    const char* fn = "atx_search_columns";
    ATX_REQUIRE(dtype == ATX_F32 || dtype == ATX_F64, ATX_EINVAL, "%s: bad dtype %d", fn, dtype);
    ATX_REQUIRE(layout == ATX_COLUMNS || layout == ATX_FIELDS, ATX_EINVAL, "%s: bad layout %d", fn, layout);
    ATX_REQUIRE(direction == ATX_SEARCH_FORWARD || direction == ATX_SEARCH_BACKWARD, ATX_EINVAL, "%s: unknown direction %d", fn, direction);
    ATX_REQUIRE(mode >= ATX_SEARCH_UP && mode <= ATX_SEARCH_MIN, ATX_EINVAL, "%s: unknown mode %d", fn, mode);
    ATX_REQUIRE(n_pts >= 0 && n_var >= 0 && n_lev >= 1 && n_tgt >= 0, ATX_EINVAL, "%s: bad sizes n_pts=%lld n_var=%lld n_lev=%lld n_tgt=%lld", fn,
                (long long)n_pts, (long long)n_var, (long long)n_lev, (long long)n_tgt);
    const bool extremum = mode >= ATX_SEARCH_MAX;
    ATX_REQUIRE(!extremum || n_tgt <= 1, ATX_EINVAL, "%s: an extremum has one result, n_tgt=%lld", fn, (long long)n_tgt);
    const int64_t n_out = n_var + (level_values != nullptr ? 1 : 0);
    ATX_REQUIRE(n_out > 0 || count != nullptr, ATX_EINVAL, "%s: no variable, no level_values and no count: nothing would be written", fn);
    ATX_REQUIRE(n_lev <= kSearchMaxLevels, ATX_ENOTIMPL, "%s: n_lev=%lld exceeds the %d levels of one call", fn, (long long)n_lev, kSearchMaxLevels);
    ATX_REQUIRE(n_pts <= INT32_MAX && n_out <= 65535 && n_tgt <= 65535 && n_var * n_lev <= 65535 && n_out * n_tgt <= 65535 && n_pts * n_tgt <= INT32_MAX,
                ATX_ENOTIMPL, "%s: sizes exceed the indexing of one launch (n_pts=%lld n_var=%lld n_lev=%lld n_tgt=%lld)", fn, (long long)n_pts,
                (long long)n_var, (long long)n_lev, (long long)n_tgt);
    if (layout == ATX_COLUMNS) {
        ATX_REQUIRE(src_pitch >= n_var * n_lev && search_pitch >= n_lev && out_pitch >= n_out * n_tgt, ATX_ESHAPE,
                    "%s: column pitch (%lld, %lld, %lld) < rows (%lld, %lld, %lld)", fn, (long long)src_pitch, (long long)search_pitch, (long long)out_pitch,
                    (long long)(n_var * n_lev), (long long)n_lev, (long long)(n_out * n_tgt));
    } else {
        ATX_REQUIRE((src_pitch >= n_pts || n_var == 0) && search_pitch >= n_pts && (out_pitch >= n_pts || n_out == 0), ATX_ESHAPE,
                    "%s: field pitch (%lld, %lld, %lld) < points %lld", fn, (long long)src_pitch, (long long)search_pitch, (long long)out_pitch, (long long)n_pts);
    }
    ATX_REQUIRE(((src || n_var == 0) && search) || n_pts == 0, ATX_EINVAL, "%s: null src / search pointer", fn);
    ATX_REQUIRE(targets || n_tgt == 0 || extremum, ATX_EINVAL, "%s: null targets", fn);
    ATX_REQUIRE(out || n_out == 0 || n_pts == 0 || n_tgt == 0, ATX_EINVAL, "%s: null out pointer", fn);
    if (n_pts == 0 || n_tgt == 0) return ATX_OK;
    const int elem = dtype == ATX_F32 ? 4 : 8;
    struct Named {
        const char* name;
        SearchExtent extent;
        bool present;
    };
    const Named inputs[] = {{"src", search_extent(src, n_pts, n_var * n_lev, src_pitch, layout, elem), n_var > 0},
                            {"search", search_extent(search, n_pts, n_lev, search_pitch, layout, elem), true},
                            {"targets", search_extent(targets, n_tgt, 1, n_tgt, ATX_FIELDS, 8), targets != nullptr && !extremum},
                            {"level_values", search_extent(level_values, n_lev, 1, n_lev, ATX_FIELDS, 8), level_values != nullptr}};
    const Named outputs[] = {{"out", search_extent(out, n_pts, n_out * n_tgt, out_pitch, layout, elem), n_out > 0},
                             {"count", search_extent(count, n_pts * n_tgt, 1, n_pts * n_tgt, ATX_FIELDS, 1), count != nullptr}};
    for (const Named& o : outputs)
        for (const Named& i : inputs) ATX_REQUIRE(!(o.present && i.present && o.extent.overlaps(i.extent)), ATX_EINVAL, "%s: %s overlaps %s", fn, o.name, i.name);
    ATX_REQUIRE(!(outputs[0].present && outputs[1].present && outputs[0].extent.overlaps(outputs[1].extent)), ATX_EINVAL, "%s: count overlaps out", fn);
    SearchCall c;
    c.src = src, c.search = search, c.out = out, c.count = count, c.targets = targets, c.level_values = level_values;
    c.n_pts = n_pts, c.src_pitch = src_pitch, c.search_pitch = search_pitch, c.out_pitch = out_pitch;
    c.n_var = (int)n_var, c.n_lev = (int)n_lev, c.n_tgt = (int)n_tgt, c.layout = layout, c.backward = direction == ATX_SEARCH_BACKWARD ? 1 : 0, c.mode = mode;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dtype == ATX_F32 ? search_typed<float>(c, s) : search_typed<double>(c, s);
}
