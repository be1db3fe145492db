// Reductions over a field or a stack: minimum, maximum, both in one pass, and the NaN count.
//
// Replaces the range and validity checks of the reference
//   R: filters/fields/cos_sin_from_rad.py:73-76            data.min() then data.max()
//   R: tests/field_filters/test_apply_mask.py:106          np.sum(np.isnan(result))
// by ONE pass over the data with 16-byte non-temporal loads (HBM-bound on a stack, launch-bound on one field) and a two-level
// finish: with a caller's workspace every workgroup stores its partials and a second, one-workgroup launch combines them, so the
// result may be a pinned host cell; without one the workgroups combine through atomics on a device cell.
#include "atx_common.hpp"

namespace atx {

__device__ __forceinline__ void atomic_minmax(double* addr, double v, bool is_max) {
    unsigned long long* a = reinterpret_cast<unsigned long long*>(addr);
    unsigned long long old = *a;
    while (true) {
        const double cur = __longlong_as_double((long long)old);
        if (cur != cur) return;  // already NaN: np.min/np.max propagate it
        double nv;
        if (v != v) nv = v;
        else nv = is_max ? (v > cur ? v : cur) : (v < cur ? v : cur);
        const unsigned long long nb = (unsigned long long)__double_as_longlong(nv);
        if (nb == old) return;
        const unsigned long long prev = atomicCAS(a, old, nb);
        if (prev == old) return;
        old = prev;
    }
}

__global__ void reduce_init_kernel(double* result, int red) {
    if (red == ATX_RED_MINMAX) {
        result[0] = INFINITY;
        result[1] = -INFINITY;
        return;
    }
    *result = red == ATX_RED_MIN ? INFINITY : (red == ATX_RED_MAX ? -INFINITY : 0.0);
}

// One partial per lane over a grid-stride sweep (4 independent loads in flight), 64-lane shuffle, one LDS combine per
// workgroup, ONE atomic per workgroup (a per-wave atomic on a single address serialised 100 k of them on large inputs).
constexpr int kRedUnroll = 4;
// Workgroup cap = partial slots of the two-level finish.  137 levels of O1280 against 8192: f64 min+max 0.707 -> 0.74, NaN count f32 0.70 -> 0.74,
// f64 0.715 -> 0.76, f32 min+max unchanged (0.68); 65536 loses (f32 min+max 0.60); one field is far below either cap.  profiles/r04_reduce_grid.log
constexpr int64_t kRedGrid = 32768;

__device__ __forceinline__ double red_combine(double a, double b, int red) {
    if (red == ATX_RED_NANCOUNT) return a + b;
    if (a != a || b != b) return NAN;  // np.min / np.max propagate NaN
    if (red == ATX_RED_MIN) return b < a ? b : a;
    return b > a ? b : a;
}

// Two-level finish WITHOUT one atomic per workgroup on the result (a CAS loop on one address: 1 600 workgroups over one 26 MB
// field spent 10 us of a 43 us call in it, min AND max 30 us) and without an initialisation launch: with a caller-provided workspace
// every workgroup stores its partial(s) with plain stores, and a second, one-workgroup launch (reduce_final_kernel) combines them and
// writes `result` — which may then be a pinned HOST cell: no copy back either.  The kernel boundary is the only synchronisation.
// (Round 3 first tried a single launch with a ticket — the last workgroup to arrive combines — and measured it SLOWER than the
// atomics: the device-scope release every workgroup needs before taking its ticket writes the XCD's L2 back; 43 -> 60 us for one
// field, 0.66 -> 1.0 ms for a 137-level stack.  profiles/r03_small_calls.log.)
struct RedWorkspace {
    double a[kRedGrid];
    double b[kRedGrid];
};

__global__ void __launch_bounds__(kBlock)
reduce_final_kernel(const RedWorkspace* __restrict__ ws, int n, int ra, int red, double* result) {
    __shared__ double fa[kBlock / kWave], fb[kBlock / kWave];
    const double id_a = ra == ATX_RED_MIN ? INFINITY : (ra == ATX_RED_MAX ? -INFINITY : 0.0);
    double a = id_a, b = -INFINITY;
    for (int i = threadIdx.x; i < n; i += kBlock) {
        a = red_combine(a, ws->a[i], ra);
        if (red == ATX_RED_MINMAX) b = red_combine(b, ws->b[i], ATX_RED_MAX);
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        a = red_combine(a, __shfl_down(a, off, kWave), ra);
        if (red == ATX_RED_MINMAX) b = red_combine(b, __shfl_down(b, off, kWave), ATX_RED_MAX);
    }
    if ((threadIdx.x & (kWave - 1)) == 0) {
        fa[threadIdx.x / kWave] = a;
        fb[threadIdx.x / kWave] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double xa = fa[0], xb = fb[0];
        for (int w = 1; w < kBlock / kWave; ++w) {
            xa = red_combine(xa, fa[w], ra);
            xb = red_combine(xb, fb[w], ATX_RED_MAX);
        }
        result[0] = xa;
        if (red == ATX_RED_MINMAX) result[1] = xb;
        __threadfence_system();  // `result` may live in pinned host memory
    }
}

template <typename T>
__global__ void __launch_bounds__(kBlock)
reduce_kernel(const T* __restrict__ x, int64_t n_rows, int64_t row_len, int64_t pitch, int red, double* result, double* partials) {
    const double identity = red == ATX_RED_MIN ? INFINITY : (red == ATX_RED_MAX ? -INFINITY : 0.0);
    double acc = identity;
    // rows of `row_len` elements `pitch` apart; (row, col) advances by the grid stride without a division per element
    const int64_t first = (int64_t)blockIdx.x * kBlock + threadIdx.x, stride = (int64_t)gridDim.x * kBlock;
    const int64_t d_row = stride / row_len, d_col = stride - d_row * row_len;
    int64_t row = first / row_len, col = first - row * row_len;
    while (row < n_rows) {
        T v[kRedUnroll];
        bool ok[kRedUnroll];
#pragma unroll
        for (int u = 0; u < kRedUnroll; ++u) {
            ok[u] = row < n_rows;
            v[u] = ok[u] ? x[row * pitch + col] : T(0);
            row += d_row;
            col += d_col;
            if (col >= row_len) {
                col -= row_len;
                ++row;
            }
        }
#pragma unroll
        for (int u = 0; u < kRedUnroll; ++u) {
            if (!ok[u]) continue;
            const double d = (double)v[u];
            if (red == ATX_RED_NANCOUNT) acc += (d != d) ? 1.0 : 0.0;
            else acc = red_combine(acc, d, red);
        }
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) acc = red_combine(acc, __shfl_down(acc, off, kWave), red);
    __shared__ double partial[kBlock / kWave];
    if ((threadIdx.x & (kWave - 1)) == 0) partial[threadIdx.x / kWave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = partial[0];
        for (int w = 1; w < kBlock / kWave; ++w) total = red_combine(total, partial[w], red);
        if (partials) {  // one slot per workgroup of the caller's workspace (a[] — or b[] for the MAX pass of a two-pass MINMAX)
            partials[blockIdx.x] = total;
        } else if (red == ATX_RED_NANCOUNT) {
            if (total != 0.0) atomicAdd(result, total);
        } else {
            atomic_minmax(result, total, red == ATX_RED_MAX);
        }
    }
}

// The same sweep with 16-byte loads — one (row, vector) item per step, the elements of a row's last vector beyond row_len
// masked — and with ATX_RED_MINMAX both extremes in ONE pass: the range check of cos_sin_from_rad (R: cos_sin_from_rad.py:73-76,
// `data.min()` then `data.max()`) read the stack twice at 4.7 TB/s (4-byte loads); this reads it once.
template <typename T, int VEC>
__global__ void __launch_bounds__(kBlock)
reduce_vec_kernel(const T* __restrict__ x, int64_t n_rows, int64_t row_len, int C, int64_t pitch, int red, double* result, RedWorkspace* ws) {
    using V = Pack<T, VEC>;
    const bool want_min = red == ATX_RED_MIN || red == ATX_RED_MINMAX, want_max = red == ATX_RED_MAX || red == ATX_RED_MINMAX;
    double lo = INFINITY, hi = -INFINITY, count = 0.0;
    bool seen_nan = false;
    const int64_t n_items = n_rows * C;
    const int64_t first = (int64_t)blockIdx.x * kBlock + threadIdx.x, stride = (int64_t)gridDim.x * kBlock;
    const int64_t d_row = stride / C;
    const int d_col = (int)(stride - d_row * C);
    int64_t row = first / C;
    int col = (int)(first - row * C);
    for (int64_t i = first; i < n_items; i += stride * kRedUnroll) {
        V v[kRedUnroll];
        int valid[kRedUnroll];
#pragma unroll
        for (int u = 0; u < kRedUnroll; ++u) {
            const bool ok = row < n_rows;
            valid[u] = ok ? (int)min((int64_t)VEC, row_len - (int64_t)col * VEC) : 0;
            if (ok) v[u] = pw_load_nt<T, VEC>(x + row * pitch + (int64_t)col * VEC);  // read once: non-temporal (0.73 -> 0.66 ms f32, 1.33 -> 1.19 ms f64)
            row += d_row;
            col += d_col;
            if (col >= C) {
                col -= C;
                ++row;
            }
        }
#pragma unroll
        for (int u = 0; u < kRedUnroll; ++u) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                if (e < valid[u]) {
                    const double d = (double)v[u].v[e];
                    if (d != d) {
                        seen_nan = true;
                        count += 1.0;
                    } else {
                        lo = d < lo ? d : lo;
                        hi = d > hi ? d : hi;
                    }
                }
            }
        }
    }
    if (seen_nan) lo = hi = NAN;  // np.min / np.max propagate NaN
    double a = red == ATX_RED_NANCOUNT ? count : (want_min ? lo : hi), b = hi;
    const int ra = red == ATX_RED_NANCOUNT ? ATX_RED_NANCOUNT : (want_min ? ATX_RED_MIN : ATX_RED_MAX);
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        a = red_combine(a, __shfl_down(a, off, kWave), ra);
        if (red == ATX_RED_MINMAX) b = red_combine(b, __shfl_down(b, off, kWave), ATX_RED_MAX);
    }
    __shared__ double pa[kBlock / kWave], pb[kBlock / kWave];
    if ((threadIdx.x & (kWave - 1)) == 0) {
        pa[threadIdx.x / kWave] = a;
        pb[threadIdx.x / kWave] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double ta = pa[0], tb = pb[0];
        for (int w = 1; w < kBlock / kWave; ++w) {
            ta = red_combine(ta, pa[w], ra);
            tb = red_combine(tb, pb[w], ATX_RED_MAX);
        }
        if (ws) {
            ws->a[blockIdx.x] = ta;
            ws->b[blockIdx.x] = tb;
        } else if (red == ATX_RED_NANCOUNT) {
            if (ta != 0.0) atomicAdd(result, ta);
        } else {
            atomic_minmax(result, ta, !want_min);
            if (red == ATX_RED_MINMAX) atomic_minmax(result + 1, tb, true);
        }
    }
    (void)want_max;
}

// The <= 3 elements a flat array leaves after its last whole 16-byte vector, as ONE more pair of partials in the workspace
// (slot `slot`), so that the two-level finish serves this shape too: no atomics on `result`, which may be a pinned host cell.
template <typename T>
__global__ void reduce_tail_kernel(const T* __restrict__ x, int n, int red, RedWorkspace* ws, int slot) {
    double lo = INFINITY, hi = -INFINITY, count = 0.0;
    bool seen_nan = false;
    for (int i = 0; i < n; ++i) {
        const double d = (double)x[i];
        if (d != d) {
            seen_nan = true;
            count += 1.0;
        } else {
            lo = d < lo ? d : lo;
            hi = d > hi ? d : hi;
        }
    }
    if (seen_nan) lo = hi = NAN;
    const bool want_min = red == ATX_RED_MIN || red == ATX_RED_MINMAX;
    ws->a[slot] = red == ATX_RED_NANCOUNT ? count : (want_min ? lo : hi);
    ws->b[slot] = hi;
}

}  // namespace atx

using namespace atx;

static int reduce_rows(const void* x, int64_t n_rows, int64_t row_len, int64_t pitch, int red, double* result, int dtype,
                       void* workspace, size_t workspace_bytes, void* stream, const char* who) {
    ATX_REQUIRE(n_rows >= 0 && row_len >= 0, ATX_EINVAL, "%s: negative size", who);
    ATX_REQUIRE(result && (x || n_rows == 0 || row_len == 0), ATX_EINVAL, "%s: null pointer", who);  // (an empty array may have no storage)
    ATX_REQUIRE(pitch >= row_len, ATX_ESHAPE, "%s: pitch %lld shorter than a row of %lld", who, (long long)pitch, (long long)row_len);
    ATX_REQUIRE(red >= ATX_RED_MIN && red <= ATX_RED_MINMAX, ATX_EINVAL, "%s: bad reduction %d", who, red);
    ATX_REQUIRE(dtype == ATX_F32 || dtype == ATX_F64, ATX_EINVAL, "%s: bad dtype %d", who, dtype);
    ATX_REQUIRE(!workspace || workspace_bytes >= sizeof(RedWorkspace), ATX_EWORKSPACE, "%s: workspace %zu < %zu", who, workspace_bytes,
                sizeof(RedWorkspace));
    ATX_REQUIRE(!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, ATX_EALIGN, "%s: workspace must be 8-byte aligned", who);
    hipStream_t s = static_cast<hipStream_t>(stream);
    // 16-byte loads when every row starts on a 16-byte boundary and its last (partial) vector lies inside the pitch (a flat array is
    // one row: only the base must be aligned); MINMAX exists in this form only and falls back to two scalar passes otherwise
    const int vec = dtype == ATX_F32 ? 4 : 2;
    // a flat array (one row, no pitch to hide a partial vector in): whole vectors through the vector kernel, the <= 3 elements
    // left over through the scalar one — the library never reads past x[n)
    const int64_t tail = (n_rows == 1) ? row_len % vec : 0;
    const int64_t vec_len = row_len - tail;
    const int64_t C = (vec_len + vec - 1) / vec;
    const bool vec_ok = aligned16(x) && (n_rows == 1 || (pitch % vec == 0 && C * vec <= pitch)) && C <= 0x7fffffff;
    // With a workspace EVERY shape finishes in two levels — partials with plain stores, one combining workgroup, a plain store of the
    // result, which may therefore be a pinned host cell: the single-pass case, a flat array's tail after its last whole vector (one
    // more slot), the scalar fallback's two MINMAX passes (MIN into a[], MAX into b[]) and empty input (the identities).  Without
    // one the workgroups combine through atomics on `result`, which must then be device memory (round 3 dropped the workspace for
    // every shape but the first and ran up to 8192 CAS loops over PCIe on the caller's pinned cell — the advisor's finding).
    RedWorkspace* ws = static_cast<RedWorkspace*>(workspace);
    const int ra = red == ATX_RED_NANCOUNT ? ATX_RED_NANCOUNT : ((red == ATX_RED_MIN || red == ATX_RED_MINMAX) ? ATX_RED_MIN : ATX_RED_MAX);
    if (!ws) {
        hipLaunchKernelGGL(reduce_init_kernel, dim3(1), dim3(1), 0, s, result, red);
        ATX_LAUNCH_CHECK("reduce_init");
    }
    if (n_rows == 0 || row_len == 0) {
        if (ws) {  // nothing to combine: the identities (min +inf, max -inf, count 0), as reduce_init writes them
            hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(kBlock), 0, s, ws, 0, ra, red, result);
            ATX_LAUNCH_CHECK("reduce_final");
        }
        return ATX_OK;
    }
    const int64_t grid_cap = kRedGrid - (tail > 0 ? 1 : 0);  // a tail takes one slot of the workspace
    if (vec_ok) {
        unsigned grid = 0;
        if (C > 0) {
            int64_t blocks = (n_rows * C + (int64_t)kBlock * kRedUnroll - 1) / ((int64_t)kBlock * kRedUnroll);
            grid = (unsigned)(blocks > grid_cap ? grid_cap : (blocks < 1 ? 1 : blocks));
            if (dtype == ATX_F32)
                hipLaunchKernelGGL((reduce_vec_kernel<float, 4>), dim3(grid), dim3(kBlock), 0, s, static_cast<const float*>(x), n_rows, vec_len, (int)C, pitch, red, result, ws);
            else
                hipLaunchKernelGGL((reduce_vec_kernel<double, 2>), dim3(grid), dim3(kBlock), 0, s, static_cast<const double*>(x), n_rows, vec_len, (int)C, pitch, red, result, ws);
            ATX_LAUNCH_CHECK("reduce_vec");
        }
        if (tail > 0) {
            const size_t esz = dtype == ATX_F32 ? 4 : 8;
            const void* xt = static_cast<const char*>(x) + (size_t)vec_len * esz;
            if (ws) {
                if (dtype == ATX_F32)
                    hipLaunchKernelGGL(reduce_tail_kernel<float>, dim3(1), dim3(1), 0, s, static_cast<const float*>(xt), (int)tail, red, ws, (int)grid);
                else
                    hipLaunchKernelGGL(reduce_tail_kernel<double>, dim3(1), dim3(1), 0, s, static_cast<const double*>(xt), (int)tail, red, ws, (int)grid);
                grid += 1;
            } else {  // combines into the same result cells (atomics): MINMAX as min -> result[0], max -> result[1]
                for (int pass = 0; pass < (red == ATX_RED_MINMAX ? 2 : 1); ++pass) {
                    const int r = red == ATX_RED_MINMAX ? (pass == 0 ? ATX_RED_MIN : ATX_RED_MAX) : red;
                    if (dtype == ATX_F32)
                        hipLaunchKernelGGL(reduce_kernel<float>, dim3(1), dim3(kBlock), 0, s, static_cast<const float*>(xt), (int64_t)1, tail, tail, r, result + pass, (double*)nullptr);
                    else
                        hipLaunchKernelGGL(reduce_kernel<double>, dim3(1), dim3(kBlock), 0, s, static_cast<const double*>(xt), (int64_t)1, tail, tail, r, result + pass, (double*)nullptr);
                }
            }
            ATX_LAUNCH_CHECK("reduce_tail");
        }
        if (ws) {
            hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(kBlock), 0, s, ws, (int)grid, ra, red, result);
            ATX_LAUNCH_CHECK("reduce_final");
        }
        return ATX_OK;
    }
    // scalar form (unaligned base or pitch): one pass, or MIN then MAX for MINMAX
    int64_t blocks = (n_rows * row_len + (int64_t)kBlock * kRedUnroll - 1) / ((int64_t)kBlock * kRedUnroll);
    const unsigned grid = (unsigned)(blocks > kRedGrid ? kRedGrid : (blocks < 1 ? 1 : blocks));
    for (int pass = 0; pass < (red == ATX_RED_MINMAX ? 2 : 1); ++pass) {
        const int r = red == ATX_RED_MINMAX ? (pass == 0 ? ATX_RED_MIN : ATX_RED_MAX) : red;
        double* partials = ws ? (pass == 0 ? ws->a : ws->b) : nullptr;
        if (dtype == ATX_F32)
            hipLaunchKernelGGL(reduce_kernel<float>, dim3(grid), dim3(kBlock), 0, s, static_cast<const float*>(x), n_rows, row_len, pitch, r, result + pass, partials);
        else
            hipLaunchKernelGGL(reduce_kernel<double>, dim3(grid), dim3(kBlock), 0, s, static_cast<const double*>(x), n_rows, row_len, pitch, r, result + pass, partials);
    }
    ATX_LAUNCH_CHECK("reduce");
    if (ws) {
        hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(kBlock), 0, s, ws, (int)grid, ra, red, result);
        ATX_LAUNCH_CHECK("reduce_final");
    }
    return ATX_OK;
}

extern "C" size_t atx_reduce_workspace(void) { return sizeof(RedWorkspace); }

extern "C" int atx_reduce(const void* x, int64_t n, int red, double* result, int dtype, void* workspace, size_t workspace_bytes, void* stream) {
    return reduce_rows(x, 1, n, n, red, result, dtype, workspace, workspace_bytes, stream, "atx_reduce");
}

extern "C" int atx_reduce_stack(const void* x, int64_t n_pts, int64_t n_lev, int64_t pitch, int red, double* result,
                                int dtype, int layout, void* workspace, size_t workspace_bytes, void* stream) {
    ATX_REQUIRE(layout == ATX_COLUMNS || layout == ATX_FIELDS, ATX_EINVAL, "atx_reduce_stack: bad layout %d", layout);
    if (layout == ATX_COLUMNS) return reduce_rows(x, n_pts, n_lev, pitch, red, result, dtype, workspace, workspace_bytes, stream, "atx_reduce_stack");
    return reduce_rows(x, n_lev, n_pts, pitch, red, result, dtype, workspace, workspace_bytes, stream, "atx_reduce_stack");
}
