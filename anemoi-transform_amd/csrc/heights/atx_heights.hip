// Model levels to height levels: atx_heights_interpolate (include/atx_heights.h holds the statement), built into a library of its own,
// lib/libatx_heights.so — the entry points and the kernels of libatx_levels and libatx_geopotential are fixed, tested sets, as libatx's
// are.  The coordinate the targets are given in, the geopotential c[k] of the full levels, is itself an integral of the column: the
// hydrostatic sum of atx_geopotential.hip, the bracket search of atx_levels.hip and the interpolation of every variable are ONE launch
// here, and c is never written to HBM.  The terms are a copy of geo_terms' statements: the libraries share no code beyond the headers
// under csrc/.
//
// ATX_COLUMNS, a 256-lane workgroup per tile of PT consecutive points (atx_column_tile.hpp), the phases in order:
//   1. stage     the tile's t columns and its q columns into LDS (stage_columns, the route decided per stack); A and B of the
//                n_lev + 1 half levels the rows touch; one lane per point: sp and z0 (0.0, or zs above the sea), float64;
//   2. terms     one lane per (point, level): (alpha r) t and (delta r) t into LDS — the logarithm and the two divisions, 256 lanes
//                wide.  A float64 stack's terms take the places of the t and q they were made of; a float32 stack's go to two float64
//                arrays of their own, with an odd pitch;
//   3. sum       one lane per point, from the ground up: the sequential chain of adds with kHgtBatch LDS reads in flight ahead of it,
//                as in atx_geopotential.hip; then, one lane per (point, level) again, c[k] = z0 + (S[k] + a[k]) into the place of a[k],
//                float64, and the point's flag "c never increases towards the ground and holds no NaN";
//   4. brackets  one lane per (point, target): where the flag holds, the count over the whole column IS what a bisection finds, 8 LDS
//                reads for 137 levels; any other column is counted level by level, as the statement is written — then a, b and w,
//                ONCE per pair, kept in LDS for all n_var variables;
//   5. variables the columns of t, q and of the delta terms are dead by now: their LDS (the "x region", which starts the carve) takes
//                the variables' columns, `chunk` of them at a time — as many as the region holds, one at least — staged as t and q
//                were; then one lane per output element of the chunk, in output order: two LDS reads, y = x[a] + w (x[b] - x[a]), one
//                store.  The first chunk's loads are issued before the brackets are computed.
// The LDS of a tile does not depend on n_var, so PT does not either (tile_points over HeightsCarve): four float64 variables of 137
// levels staged at once would leave 4 points to a tile, and 4 lanes to the sum phase.  ATX_FIELDS: one lane per (point, target), the
// plain reading of the statement: it walks the column from the ground once to count and once more, as far as level a, for c[a] and
// c[b]; 2 x n_var loads and n_var coalesced stores.  Both layouts and every load route evaluate the same float64 statements in the same
// order: same bits.  No scratch (profiles/heights_resources.json).
#include "../../../include/atx_heights.h"
#include "../atx_column_tile.hpp"

namespace atx {

constexpr int kHgtMaxLevels = ATX_HEIGHTS_MAX_LEVELS;
constexpr int kHgtBatch = 8;                        // LDS reads of the sum phase in flight ahead of the dependent adds
constexpr double kHgtRd = 287.0597, kHgtRv = 461.5250;  // J / (kg K), as in atx_geopotential.hip
constexpr double kHgtLn2 = 0.6931471805599453;      // alpha of the IFS top level

// The two terms of one (point, level), the statement of include/atx_geopotential.h: `a` = (alpha r) t, `d` = (delta r) t (0.0 and unused at j == 0).
struct HeightTerms {
    double a, d;
};
__device__ __forceinline__ HeightTerms height_terms(int j, double p_up, double p_dn, double t, double q) {
    const double om = 1.0 - q;
    const double dry = kHgtRd * om, wet = kHgtRv * q;
    const double r = dry + wet;
    HeightTerms g;
    if (j == 0) {
        g.a = (kHgtLn2 * r) * t;
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
__device__ __forceinline__ double level_geopotential(double z0, double below, double own) {
    const double lower = below + own;
    return z0 + lower;
}

struct HeightBracket {
    int a, b;  // a < 0: NaN;  a == b: a copy of row a;  else the interior of (a, b)
    double w;
};

// The statement of include/atx_heights.h after the count: `c(k)` gives c[k] of the point, c_ground is c[n - 1].
template <typename F>
__device__ __forceinline__ HeightBracket make_bracket(int n_below, int n, double G, double sp, double z0, double c_ground, int outside, F&& c) {
    HeightBracket r;
    r.a = r.b = -1;
    r.w = 0.0;
    if (sp != sp || z0 != z0) return r;
    if (n_below == n) {
        if (outside == ATX_HEIGHTS_NEAREST) r.a = r.b = 0;
    } else if (n_below > 0) {
        r.b = n - n_below;
        r.a = r.b - 1;
        const double ca = c(r.a), cb = c(r.b);
        const double above = ca - G, layer = ca - cb;
        r.w = above / layer;  // IEEE division
    } else if (c_ground == c_ground) {
        if (G >= z0 || outside == ATX_HEIGHTS_NEAREST) r.a = r.b = n - 1;
    }
    return r;
}

template <typename T>
__device__ __forceinline__ T interpolate(const HeightBracket& r, T xa, T xb) {
    if (r.a < 0) return quiet_nan<T>();
    if (r.a == r.b) return xa;
    const double a = (double)xa, b = (double)xb;
    const double d = b - a;
    const double s = r.w * d;  // (-ffp-contract=off: a multiply and an add)
    return (T)(a + s);
}

// The elements the staged window of `count` variables from variable v0 on covers at most, for a stack staged V elements per load: it
// starts at the vector that holds row v0 * n_lev and ends with the one that holds the last row.
__host__ __device__ inline int window_bound(int count, int n_lev, int V) { return (count * n_lev + 2 * (V - 1)) / V * V; }

// Where the LDS of a tile of `pt` points holds what (byte offsets, multiples of 16): one definition for the launch and the kernel.
// The x region starts at 0 and holds what is dead once c is there — float64: the staged q columns, which become the delta terms;
// float32: the staged t and q columns and the delta terms — and then the variables' columns.  `ta` (the alpha terms, then c) follows it:
// float64: the staged t columns, in place.
struct HeightsCarve {
    int64_t t, q, ta, td, x_bytes, sps, z0s, bw, ba, bb, mono, coef, total;
    int pa, pd;  // elements between two points' terms
};
__host__ __device__ inline HeightsCarve heights_carve(int64_t pt, int lt, int lq, int elem, int n_lev, int n_tgt, int x_least) {
    HeightsCarve c;
    int64_t end;
    if (elem == 8) {
        c.q = 0, c.td = 0, c.pd = lq;
        end = round16(pt * lq * 8);
    } else {
        c.pa = c.pd = n_lev | 1;                   // odd: the points of the sum phase fall into different banks
        c.t = 0;                                   // T [pt][lt]
        c.q = round16(pt * lt * elem);             // T [pt][lq]
        c.td = c.q + round16(pt * lq * elem);      // double [pt][pd]
        end = c.td + round16(pt * c.pd * 8);
    }
    const int64_t one = round16(pt * x_least * elem);  // one variable's window at least
    c.x_bytes = end > one ? end : one;
    end = c.x_bytes;
    if (elem == 8) {
        c.t = c.ta = end, c.pa = lt;               // T [pt][lt], then the alpha terms, then c
        end = c.t + round16(pt * lt * 8);
    } else {
        c.ta = end;                                // double [pt][pa]
        end = c.ta + round16(pt * c.pa * 8);
    }
    c.sps = end;                                   // double [pt]
    c.z0s = c.sps + round16(pt * 8);               // double [pt]
    c.bw = c.z0s + round16(pt * 8);                // double [pt][n_tgt]
    c.ba = c.bw + round16(pt * n_tgt * 8);         // int [pt][n_tgt]
    c.bb = c.ba + round16(pt * n_tgt * 4);         // int [pt][n_tgt]
    c.mono = c.bb + round16(pt * n_tgt * 4);       // int [pt]
    c.coef = c.mono + round16(pt * 4);             // double [2][n_lev + 1]
    c.total = c.coef + round16((int64_t)2 * (n_lev + 1) * 8);
    return c;
}

// ---- ATX_COLUMNS ---------------------------------------------------------------------------------------------------------------------
// VT, VQ, VX: elements per load of the staging of t, of q and of src (Vec16<T>::N, or 1 for an odd pitch or an unaligned base); lt, lq:
// elements between the columns of two points in LDS; chunk: the variables staged at a time.
template <typename T, int VT, int VQ, int VX>
__global__ void __launch_bounds__(kTileBlock)
heights_columns_kernel(const T* __restrict__ src, T* __restrict__ out, const T* __restrict__ t, const T* __restrict__ q, const T* __restrict__ sp,
                       const T* __restrict__ zs, const double* __restrict__ A, const double* __restrict__ B, const double* __restrict__ targets,
                       int64_t n_pts, int n_var, int n_lev, int n_tgt, int first, int64_t src_pitch, int64_t t_pitch, int64_t q_pitch,
                       int64_t out_pitch, int PT, int lt, int lq, int chunk, int outside) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const HeightsCarve lds = heights_carve(PT, lt, lq, (int)sizeof(T), n_lev, n_tgt, window_bound(1, n_lev, VX));
    T* xs = reinterpret_cast<T*>(smem);
    T* ts = reinterpret_cast<T*>(smem + lds.t);
    T* qs = reinterpret_cast<T*>(smem + lds.q);
    double* ta = reinterpret_cast<double*>(smem + lds.ta);  // the alpha terms, then c
    double* td = reinterpret_cast<double*>(smem + lds.td);
    double* sps = reinterpret_cast<double*>(smem + lds.sps);
    double* z0s = reinterpret_cast<double*>(smem + lds.z0s);
    double* bw = reinterpret_cast<double*>(smem + lds.bw);
    int* ba = reinterpret_cast<int*>(smem + lds.ba);
    int* bb = reinterpret_cast<int*>(smem + lds.bb);
    int* mono = reinterpret_cast<int*>(smem + lds.mono);  // 1: the point's c never increases towards the ground and holds no NaN
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
        z0s[pt] = zs ? (double)zs[p0 + pt] : 0.0;
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
        const HeightTerms g = height_terms(first + k, p_up, p_dn, tk, qk);
        ta[pt * pa + k] = g.a;  // (float64: the places of tk and qk, which only this lane reads)
        td[pt * pd + k] = g.d;
    }
    __syncthreads();
    // 3. sum: S[k], the sum of d over the levels below k, replaces d[k] ...
    for (int pt = tid; pt < npt; pt += kTileBlock) {
        double* d = td + pt * pd;
        double S = 0.0;
        int k = n_lev - 1;
        for (; k >= kHgtBatch - 1; k -= kHgtBatch) {  // a batch of reads, then the dependent adds, then the writes
            double v[kHgtBatch];
#pragma unroll
            for (int i = 0; i < kHgtBatch; ++i) v[i] = d[k - i];
#pragma unroll
            for (int i = 0; i < kHgtBatch; ++i) {
                const double below = S;
                S = S + v[i];
                v[i] = below;
            }
#pragma unroll
            for (int i = 0; i < kHgtBatch; ++i) d[k - i] = v[i];
        }
        for (; k >= 0; --k) {
            const double below = S;
            S = S + d[k];  // (j == 0 adds 0.0 to a sum nothing reads again)
            d[k] = below;
        }
    }
    __syncthreads();
    // ... c[k] replaces a[k] ...
    TileWalk level(tid, n_lev);
    for (int i = tid; i < npt * n_lev; i += kTileBlock, level.next()) {
        const int pt = level.row, k = level.col;
        ta[pt * pa + k] = level_geopotential(z0s[pt], td[pt * pd + k], ta[pt * pa + k]);
    }
    __syncthreads();
    // ... and the flag; the x region is free from here on: the first chunk of variables is on its way while the brackets are made
    TileWalk pair(tid, n_lev);
    for (int i = tid; i < npt * n_lev; i += kTileBlock, pair.next()) {
        const int pt = pair.row, k = pair.col;
        if (k + 1 < n_lev && !(ta[pt * pa + k] >= ta[pt * pa + k + 1])) mono[pt] = 0;  // (a NaN fails too — one level alone counts the same either way; every lane that writes, writes 0)
    }
    auto stage_chunk = [&](int v0, int count, int& from, int& width) {
        from = v0 * n_lev / VX * VX;
        const int to = ((v0 + count) * n_lev + VX - 1) / VX * VX;  // (the 16-byte route: inside the pitch, column_route has seen to it)
        width = to - from;
        stage_columns<T, VX>(src + from, xs, p0, npt, src_pitch, width, tid);
    };
    int from = 0, width = 0;
    stage_chunk(0, chunk < n_var ? chunk : n_var, from, width);
    __syncthreads();
    // 4. brackets
    TileWalk bracket(tid, n_tgt);
    for (int i = tid; i < npt * n_tgt; i += kTileBlock, bracket.next()) {
        const int pt = bracket.row;
        const double G = targets[bracket.col];
        const double* col = ta + pt * pa;
        int n_below = 0;
        if (mono[pt]) {  // #{k : col[k] < G} of a column that never increases: n_lev - (the first k with col[k] < G) (a NaN target: 0)
            int lo = 0, hi = n_lev;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (col[mid] < G)
                    hi = mid;
                else
                    lo = mid + 1;
            }
            n_below = n_lev - lo;
        } else {
            for (int k = 0; k < n_lev; ++k) n_below += col[k] < G ? 1 : 0;
        }
        const HeightBracket r = make_bracket(n_below, n_lev, G, sps[pt], z0s[pt], col[n_lev - 1], outside, [&](int k) { return col[k]; });
        ba[i] = r.a;
        bb[i] = r.b;
        bw[i] = r.w;
    }
    __syncthreads();
    // 5. variables
    for (int v0 = 0; v0 < n_var; v0 += chunk) {
        const int count = n_var - v0 < chunk ? n_var - v0 : chunk;
        if (v0 > 0) {
            __syncthreads();  // the chunk before has been applied
            stage_chunk(v0, count, from, width);
            __syncthreads();
        }
        const int per_point = count * n_tgt;
        const int lead = v0 * n_lev - from;  // the window starts at a vector, the chunk's first row `lead` elements into it
        TileWalk apply(tid, per_point);
        for (int i = tid; i < npt * per_point; i += kTileBlock, apply.next()) {
            const int pt = apply.row, j = apply.col;
            const int v = j / n_tgt, tg = j - v * n_tgt;
            HeightBracket r;
            r.a = ba[pt * n_tgt + tg];
            r.b = bb[pt * n_tgt + tg];
            r.w = bw[pt * n_tgt + tg];
            const T* x = xs + pt * width + lead + v * n_lev;
            const T xa = x[r.a < 0 ? 0 : r.a], xb = x[r.b < 0 ? 0 : r.b];
            out[(p0 + pt) * out_pitch + v0 * n_tgt + j] = interpolate<T>(r, xa, xb);
        }
    }
}

// ---- ATX_FIELDS ----------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(kTileBlock)
heights_fields_kernel(const T* __restrict__ src, T* __restrict__ out, const T* __restrict__ t, const T* __restrict__ q, const T* __restrict__ sp,
                      const T* __restrict__ zs, const double* __restrict__ A, const double* __restrict__ B, const double* __restrict__ targets,
                      int64_t n_pts, int n_var, int n_lev, int n_tgt, int first, int64_t src_pitch, int64_t t_pitch, int64_t q_pitch,
                      int64_t out_pitch, int outside) {
    const int64_t p = (int64_t)blockIdx.x * kTileBlock + threadIdx.x;
    if (p >= n_pts) return;
    const int tg = blockIdx.y;
    const double s = (double)sp[p];
    const double z0 = zs ? (double)zs[p] : 0.0;
    const double G = targets[tg];
    // the column from the ground up (k is uniform: scalar loads of A, B), once to count ...
    auto walk = [&](int top, auto&& seen) {
        double S = 0.0;
        for (int k = n_lev - 1; k >= top; --k) {
            const int j = first + k;
            const double p_up = half_level(A, B, j, s), p_dn = half_level(A, B, j + 1, s);
            const HeightTerms g = height_terms(j, p_up, p_dn, (double)t[(int64_t)k * t_pitch + p], (double)q[(int64_t)k * q_pitch + p]);
            seen(k, level_geopotential(z0, S, g.a));
            S = S + g.d;
        }
    };
    int n_below = 0;
    double c_ground = 0.0;
    walk(0, [&](int k, double c) {
        if (k == n_lev - 1) c_ground = c;
        n_below += c < G ? 1 : 0;
    });
    // ... and, for an interior target, once more as far as level a for c[a] and c[b]
    double ca = 0.0, cb = 0.0;
    if (n_below > 0 && n_below < n_lev) {
        const int b = n_lev - n_below;
        walk(b - 1, [&](int k, double c) {
            if (k == b) cb = c;
            if (k == b - 1) ca = c;
        });
    }
    const HeightBracket r = make_bracket(n_below, n_lev, G, s, z0, c_ground, outside, [&](int k) { return k == n_lev - n_below ? cb : ca; });
    const int a = r.a < 0 ? 0 : r.a, b = r.b < 0 ? 0 : r.b;
    for (int v = 0; v < n_var; ++v) {
        const T xa = src[((int64_t)v * n_lev + a) * src_pitch + p], xb = src[((int64_t)v * n_lev + b) * src_pitch + p];
        out[((int64_t)v * n_tgt + tg) * out_pitch + p] = interpolate<T>(r, xa, xb);
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
struct HeightsCall {
    const void *src, *t, *q, *sp, *zs;
    void* out;
    const double *A, *B, *targets;
    int64_t n_pts, src_pitch, t_pitch, q_pitch, out_pitch;
    int n_var, n_lev, n_tgt, first, layout, outside;
};

template <typename T>
static int heights_typed(const HeightsCall& c, hipStream_t st) {
    const char* fn = "atx_heights_interpolate";
    const T* src = static_cast<const T*>(c.src);
    const T* t = static_cast<const T*>(c.t);
    const T* q = static_cast<const T*>(c.q);
    const T* sp = static_cast<const T*>(c.sp);
    const T* zs = static_cast<const T*>(c.zs);
    T* out = static_cast<T*>(c.out);
    if (c.layout == ATX_FIELDS) {
        const dim3 grid((unsigned)((c.n_pts + kTileBlock - 1) / kTileBlock), (unsigned)c.n_tgt);
        hipLaunchKernelGGL((heights_fields_kernel<T>), grid, dim3(kTileBlock), 0, st, src, out, t, q, sp, zs, c.A, c.B, c.targets, c.n_pts, c.n_var,
                           c.n_lev, c.n_tgt, c.first, c.src_pitch, c.t_pitch, c.q_pitch, c.out_pitch, c.outside);
        ATX_LAUNCH_CHECK("heights_fields");
        return ATX_OK;
    }
    constexpr int VEC = Vec16<T>::N;
    const ColumnRoute rt = column_route<VEC>(c.t, c.t_pitch, c.n_lev), rq = column_route<VEC>(c.q, c.q_pitch, c.n_lev);
    const ColumnRoute rx = column_route<VEC>(c.src, c.src_pitch, c.n_var * c.n_lev);
    const int lt = rt.lds_pitch, lq = rq.lds_pitch, vx = rx.vector ? VEC : 1;
    auto carve = [&](int64_t pt) { return heights_carve(pt, lt, lq, (int)sizeof(T), c.n_lev, c.n_tgt, window_bound(1, c.n_lev, vx)); };
    auto bytes = [&](int64_t pt) { return carve(pt).total; };
    const int PT = tile_points(bytes);
    ATX_REQUIRE(PT > 0, ATX_ENOTIMPL, "%s: one point's %d levels and %d targets need %lld bytes of LDS, a workgroup has %lld", fn, c.n_lev, c.n_tgt,
                (long long)bytes(1), (long long)kTileLdsLimit);
    int chunk = 1;  // the variables the x region holds at a time
    while (chunk < c.n_var && (int64_t)PT * window_bound(chunk + 1, c.n_lev, vx) * (int64_t)sizeof(T) <= carve(PT).x_bytes) ++chunk;
    const int64_t tiles = (c.n_pts + PT - 1) / PT;
    const size_t lds = (size_t)bytes(PT);
    with_flag(rt.vector, [&](auto vec_t) {
        return with_flag(rq.vector, [&](auto vec_q) {
            return with_flag(rx.vector, [&](auto vec_x) {
                constexpr int VT = decltype(vec_t)::value ? VEC : 1, VQ = decltype(vec_q)::value ? VEC : 1, VX = decltype(vec_x)::value ? VEC : 1;
                hipLaunchKernelGGL((heights_columns_kernel<T, VT, VQ, VX>), dim3((unsigned)tiles), dim3(kTileBlock), lds, st, src, out, t, q, sp, zs, c.A,
                                   c.B, c.targets, c.n_pts, c.n_var, c.n_lev, c.n_tgt, c.first, c.src_pitch, c.t_pitch, c.q_pitch, c.out_pitch, PT, lt,
                                   lq, chunk, c.outside);
                return 0;
            });
        });
    });
    ATX_LAUNCH_CHECK("heights_columns");
    return ATX_OK;
}

// The bytes [lo, hi) a stack of `rows` rows touches.
static void heights_extent(const void* base, int64_t n_pts, int64_t rows, int64_t pitch, int layout, int elem, uintptr_t& lo, uintptr_t& hi) {
    const int64_t elements = layout == ATX_COLUMNS ? (n_pts - 1) * pitch + rows : (rows - 1) * pitch + n_pts;
    lo = reinterpret_cast<uintptr_t>(base);
    hi = lo + (uintptr_t)elements * (uintptr_t)elem;
}

}  // namespace atx

using namespace atx;

extern "C" int atx_heights_version(void) { return ATX_HEIGHTS_VERSION; }

extern "C" const char* atx_heights_last_error(void) { return last_error().c_str(); }

extern "C" int atx_heights_interpolate(const void* src, void* out, const void* t, const void* q, const void* sp, const void* zs, const double* A,
                                       const double* B, const double* targets, int64_t n_pts, int64_t n_var, int64_t n_lev, int64_t n_tgt,
                                       int64_t n_half, int64_t src_pitch, int64_t t_pitch, int64_t q_pitch, int64_t out_pitch, int dtype, int layout,
                                       int reference, int outside, void* stream) {
    const char* fn = "atx_heights_interpolate";
    ATX_REQUIRE(dtype == ATX_F32 || dtype == ATX_F64, ATX_EINVAL, "%s: bad dtype %d", fn, dtype);
    ATX_REQUIRE(layout == ATX_COLUMNS || layout == ATX_FIELDS, ATX_EINVAL, "%s: bad layout %d", fn, layout);
    ATX_REQUIRE(reference == ATX_HEIGHTS_ABOVE_GROUND || reference == ATX_HEIGHTS_ABOVE_SEA, ATX_EINVAL, "%s: unknown reference %d", fn, reference);
    ATX_REQUIRE(outside == ATX_HEIGHTS_NEAREST || outside == ATX_HEIGHTS_MISSING, ATX_EINVAL, "%s: unknown outside policy %d", fn, outside);
    ATX_REQUIRE(n_pts >= 0 && n_var >= 1 && n_lev >= 1 && n_tgt >= 0, ATX_EINVAL, "%s: bad sizes n_pts=%lld n_var=%lld n_lev=%lld n_tgt=%lld", fn,
                (long long)n_pts, (long long)n_var, (long long)n_lev, (long long)n_tgt);
    ATX_REQUIRE(n_half >= 2, ATX_EINVAL, "%s: n_half=%lld: a model has at least one level, two half levels", fn, (long long)n_half);
    ATX_REQUIRE(n_lev <= n_half - 1, ATX_EINVAL, "%s: n_lev=%lld rows are the lowest levels of a model of %lld, n_half=%lld", fn, (long long)n_lev,
                (long long)(n_half - 1), (long long)n_half);
    ATX_REQUIRE(n_lev <= kHgtMaxLevels, ATX_ENOTIMPL, "%s: n_lev=%lld exceeds the %d levels of one call", fn, (long long)n_lev, kHgtMaxLevels);
    ATX_REQUIRE(n_pts <= INT32_MAX && n_var <= 65535 && n_tgt <= 65535 && n_half <= 65535 && n_var * n_lev <= 65535 && n_var * n_tgt <= 65535, ATX_ENOTIMPL,
                "%s: sizes exceed the indexing of one launch (n_pts=%lld n_var=%lld n_lev=%lld n_tgt=%lld n_half=%lld)", fn, (long long)n_pts,
                (long long)n_var, (long long)n_lev, (long long)n_tgt, (long long)n_half);
    if (layout == ATX_COLUMNS) {
        ATX_REQUIRE(src_pitch >= n_var * n_lev && t_pitch >= n_lev && q_pitch >= n_lev && out_pitch >= n_var * n_tgt, ATX_ESHAPE,
                    "%s: column pitch (%lld, %lld, %lld, %lld) < rows (%lld, %lld, %lld, %lld)", fn, (long long)src_pitch, (long long)t_pitch,
                    (long long)q_pitch, (long long)out_pitch, (long long)(n_var * n_lev), (long long)n_lev, (long long)n_lev, (long long)(n_var * n_tgt));
    } else {
        ATX_REQUIRE(src_pitch >= n_pts && t_pitch >= n_pts && q_pitch >= n_pts && out_pitch >= n_pts, ATX_ESHAPE,
                    "%s: field pitch (%lld, %lld, %lld, %lld) < points %lld", fn, (long long)src_pitch, (long long)t_pitch, (long long)q_pitch,
                    (long long)out_pitch, (long long)n_pts);
    }
    ATX_REQUIRE(A && B, ATX_EINVAL, "%s: null A / B coefficients", fn);
    ATX_REQUIRE((src && t && q && sp) || n_pts == 0, ATX_EINVAL, "%s: null src / t / q / sp pointer", fn);
    ATX_REQUIRE(zs || reference == ATX_HEIGHTS_ABOVE_GROUND || n_pts == 0, ATX_EINVAL, "%s: null zs above the sea", fn);
    ATX_REQUIRE(targets || n_tgt == 0, ATX_EINVAL, "%s: null targets", fn);
    ATX_REQUIRE(out || n_pts == 0 || n_tgt == 0, ATX_EINVAL, "%s: null out pointer", fn);
    if (n_pts == 0 || n_tgt == 0) return ATX_OK;
    const int elem = dtype == ATX_F32 ? 4 : 8;
    uintptr_t olo, ohi, lo, hi;
    heights_extent(out, n_pts, n_var * n_tgt, out_pitch, layout, elem, olo, ohi);
    heights_extent(src, n_pts, n_var * n_lev, src_pitch, layout, elem, lo, hi);
    ATX_REQUIRE(!(olo < hi && lo < ohi), ATX_EINVAL, "%s: out overlaps src", fn);
    heights_extent(t, n_pts, n_lev, t_pitch, layout, elem, lo, hi);
    ATX_REQUIRE(!(olo < hi && lo < ohi), ATX_EINVAL, "%s: out overlaps t", fn);
    heights_extent(q, n_pts, n_lev, q_pitch, layout, elem, lo, hi);
    ATX_REQUIRE(!(olo < hi && lo < ohi), ATX_EINVAL, "%s: out overlaps q", fn);
    HeightsCall c;
    c.src = src, c.t = t, c.q = q, c.sp = sp, c.out = out;
    c.zs = reference == ATX_HEIGHTS_ABOVE_SEA ? zs : nullptr;  // above the ground: z0 = 0.0, whatever zs holds
    c.A = A, c.B = B, c.targets = targets;
    c.n_pts = n_pts, c.src_pitch = src_pitch, c.t_pitch = t_pitch, c.q_pitch = q_pitch, c.out_pitch = out_pitch;
    c.n_var = (int)n_var, c.n_lev = (int)n_lev, c.n_tgt = (int)n_tgt, c.first = (int)(n_half - 1 - n_lev), c.layout = layout, c.outside = outside;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dtype == ATX_F32 ? heights_typed<float>(c, s) : heights_typed<double>(c, s);
}
