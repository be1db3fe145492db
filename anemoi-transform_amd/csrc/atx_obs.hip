// Observation gridding: a table of scattered observations -> one gridded field per target time and column.
//
// irregular_to_grid (R: filters/tabular/irregular_to_grid.py:113-161) loops over the target times on the host; for each it selects
// the rows whose `date` lies in the window around the target (select_window, :209-254), scores them (get_nearest_obs, :256-317),
// keeps per `spatial_index` the row of smallest score — the FIRST such row of the table among equals (pandas idxmin) — and
// writes that row's values into float64 grids pre-filled with NaN (_fill_grids, :190-207).  The statement, per row r and target t:
//
//   takes part   date[r] != NaT, target[t] != NaT, not every column of r is NaN, 0 <= cell[r] < n_cells, and
//                target[t] + before  <(=)  date[r]  <(=)  target[t] + after      (each end closed or open)
//   time_score   (double)|date[r] - target[t]| / (double)freq                    (int64 ns -> float64, one IEEE division)
//   score        time_score                                       if w <= 0
//                (1.0 - w) * time_score + w * (nan_count / n_cols)  otherwise     (two products, one sum, no contraction)
//   winner[t][c] the smallest r among the rows of cell c with the smallest score, -1 when no row takes part
//
// A keyed arg-min over scattered rows, done with two order-independent minima so that the result does not depend on which wave
// arrives first:
//   pass 1  one lane per row: 64-bit unsigned atomic min of the score's BIT PATTERN into best[t][cell].  Scores are finite and
//           >= +0, and non-negative doubles order like their bit patterns.  A lane first reads best[t][cell] with a plain load
//           and skips the atomic when its score is larger: the table only ever decreases, so a stale (larger) value can only make
//           the lane issue an atomic it did not need, never drop one it did.  Rows of a crowded cell mostly stop there.
//   pass 2  the same lanes recompute the same score (same code, same bits); those that equal best[t][cell] do a 32-bit unsigned
//           atomic min of their row index into winner[t][cell].
// Both tables start as all-ones bytes (UINT64_MAX / 0xffffffff = -1), one memset each.  A cell index is compared against
// [0, n_cells) BEFORE it becomes an address; rows outside are dropped, as the reference drops them.
//
// atx_obs_fill_stack then writes level t * n_cols + c of a float64 stack: values[c][winner[t][p]], NaN where the winner is -1
// or any other value outside [0, n_obs) — in both layouts, whatever table the caller hands in.
// The reads are a gather of 8-byte words; the stores are 16-byte and non-temporal, as in the other streaming kernels:
//   ATX_FIELDS   lane = two neighbouring points of target t (grid.y = t): their winners are read once and the n_cols levels of
//                that target are written from them.
//   ATX_COLUMNS  lane = one 16-byte vector (two levels of one point); the padding of a row is written with zeros.
#include "atx_common.hpp"

namespace atx {

struct ObsWindow {
    int64_t before_ns, after_ns, freq_ns;
    int closed_before, closed_after;
    double w;
};

// PASS 1: best[t][cell] = min(score bits); PASS 2: winner[t][cell] = min(row) over the rows whose score bits equal best
template <int PASS>
__global__ void __launch_bounds__(kBlock)
obs_best_kernel(const int64_t* __restrict__ date_ns, const int64_t* __restrict__ cell, const double* __restrict__ values, int64_t n_obs,
                int n_cols, int64_t val_pitch, const int64_t* __restrict__ target_ns, int n_time, int64_t n_cells, ObsWindow win,
                unsigned long long* best, unsigned int* winner) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n_obs) return;
    const int64_t c = cell[r];
    if (c < 0 || c >= n_cells) return;  // never an address
    const int64_t d = date_ns[r];
    if (d == INT64_MIN) return;  // NaT
    int nan_count = 0;
    for (int j = 0; j < n_cols; ++j) {
        const double v = values[(int64_t)j * val_pitch + r];
        nan_count += (v != v) ? 1 : 0;
    }
    if (nan_count == n_cols) return;
    const double freq = (double)win.freq_ns;
    const double nan_score = (double)nan_count / (double)n_cols;
    for (int t = 0; t < n_time; ++t) {
        const int64_t tt = target_ns[t];
        if (tt == INT64_MIN) continue;
        const int64_t lo = tt + win.before_ns, hi = tt + win.after_ns;
        if (!(win.closed_before ? d >= lo : d > lo)) continue;
        if (!(win.closed_after ? d <= hi : d < hi)) continue;
        const int64_t diff = d - tt;
        const double time_score = (double)(diff < 0 ? -diff : diff) / freq;
        double score = time_score;
        if (win.w > 0.0) {
            const double a = (1.0 - win.w) * time_score;
            const double b = win.w * nan_score;
            score = a + b;
        }
        const unsigned long long bits = (unsigned long long)__double_as_longlong(score);
        const int64_t slot = (int64_t)t * n_cells + c;
        if constexpr (PASS == 1) {
            if (bits < __builtin_nontemporal_load(best + slot)) atomicMin(best + slot, bits);
        } else {
            if (bits == best[slot]) atomicMin(winner + slot, (unsigned int)r);
        }
    }
}

__device__ __forceinline__ double obs_value(const int32_t* __restrict__ winner, const double* __restrict__ values, int64_t n_obs,
                                            int64_t val_pitch, int64_t n_cells, int t, int c, int64_t p) {
    const int32_t w = winner[(int64_t)t * n_cells + p];
    return (w >= 0 && (int64_t)w < n_obs) ? values[(int64_t)c * val_pitch + w] : quiet_nan<double>();
}

template <int VEC>
__device__ __forceinline__ void obs_store(double* p, const Pack<double, VEC>& v) {
    if constexpr (VEC == 2) {
        typedef double NV __attribute__((ext_vector_type(2)));
        __builtin_nontemporal_store(*reinterpret_cast<const NV*>(&v), reinterpret_cast<NV*>(p));
    } else {
        __builtin_nontemporal_store(v.v[0], p);
    }
}

// ATX_FIELDS: lane = VEC neighbouring points of target blockIdx.y; points in [n_cells, pitch) are padding, written with zeros
template <int VEC>
__global__ void __launch_bounds__(kBlock)
obs_fill_fields_kernel(const int32_t* __restrict__ winner, const double* __restrict__ values, double* out, int64_t n_obs, int n_cols,
                       int64_t val_pitch, int64_t n_cells, int n_time, int64_t pitch) {
    const int64_t p0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * VEC;
    if (p0 >= pitch) return;
    bool real[VEC];  // a point of the grid; padding is told by its position, never by a value of the caller's table
#pragma unroll
    for (int e = 0; e < VEC; ++e) real[e] = p0 + e < n_cells;
    for (int t = blockIdx.y; t < n_time; t += gridDim.y) {
        int32_t w[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) w[e] = real[e] ? winner[(int64_t)t * n_cells + p0 + e] : -1;
        for (int c = 0; c < n_cols; ++c) {
            Pack<double, VEC> o;
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                if (!real[e]) o.v[e] = 0.0;
                else o.v[e] = (w[e] >= 0 && (int64_t)w[e] < n_obs) ? values[(int64_t)c * val_pitch + w[e]] : quiet_nan<double>();
            }
            obs_store<VEC>(out + ((int64_t)t * n_cols + c) * pitch + p0, o);
        }
    }
}

// ATX_COLUMNS: vector i of the stack is (point i / vpr, levels (i % vpr) * VEC ..); levels in [n_lev, pitch) are padding
template <int VEC, typename I>
__global__ void __launch_bounds__(kBlock)
obs_fill_columns_kernel(const int32_t* __restrict__ winner, const double* __restrict__ values, double* out, int64_t n_obs, int n_cols,
                        int64_t val_pitch, int64_t n_cells, int n_lev, I total, I vpr) {
    const I i = (I)blockIdx.x * (I)kBlock + (I)threadIdx.x;
    if (i >= total) return;
    const I p = i / vpr;
    const int l0 = (int)(i - p * vpr) * VEC;
    Pack<double, VEC> o;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        const int l = l0 + e;
        o.v[e] = l < n_lev ? obs_value(winner, values, n_obs, val_pitch, n_cells, l / n_cols, l % n_cols, (int64_t)p) : 0.0;
    }
    obs_store<VEC>(out + (int64_t)i * VEC, o);
}

}  // namespace atx

using namespace atx;

extern "C" int atx_obs_best_per_cell(const int64_t* date_ns, const int64_t* cell, const double* values, int64_t n_obs, int32_t n_cols,
                                     int64_t val_pitch, const int64_t* target_ns, int32_t n_time, int64_t n_cells, int64_t before_ns,
                                     int64_t after_ns, int closed_before, int closed_after, int64_t freq_ns, double w,
                                     uint64_t* best, int32_t* winner, void* stream) {
    ATX_REQUIRE(n_obs >= 0 && n_time >= 0 && n_cells >= 0 && n_cols > 0, ATX_EINVAL, "atx_obs_best_per_cell: bad sizes");
    ATX_REQUIRE(n_obs < 0x80000000ll, ATX_EINVAL, "atx_obs_best_per_cell: %lld rows do not fit an int32 row index", (long long)n_obs);
    ATX_REQUIRE(freq_ns > 0, ATX_EINVAL, "atx_obs_best_per_cell: freq_ns must be positive");
    ATX_REQUIRE(w >= 0.0 && w <= 1.0, ATX_EINVAL, "atx_obs_best_per_cell: the weight must lie in [0, 1]");
    ATX_REQUIRE(val_pitch >= n_obs, ATX_ESHAPE, "atx_obs_best_per_cell: val_pitch %lld below n_obs", (long long)val_pitch);
    const int64_t slots = (int64_t)n_time * n_cells;
    if (slots == 0) return ATX_OK;
    ATX_REQUIRE(best && winner && target_ns, ATX_EINVAL, "atx_obs_best_per_cell: null pointer");
    ATX_REQUIRE((date_ns && cell && values) || n_obs == 0, ATX_EINVAL, "atx_obs_best_per_cell: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    int st = hip_status(hipMemsetAsync(best, 0xff, (size_t)slots * sizeof(uint64_t), s), "atx_obs_best_per_cell memset");
    if (st != ATX_OK) return st;
    st = hip_status(hipMemsetAsync(winner, 0xff, (size_t)slots * sizeof(int32_t), s), "atx_obs_best_per_cell memset");
    if (st != ATX_OK) return st;
    if (n_obs == 0) return ATX_OK;
    const ObsWindow win{before_ns, after_ns, freq_ns, closed_before != 0, closed_after != 0, w};
    const dim3 grid((unsigned)((n_obs + kBlock - 1) / kBlock));
    unsigned long long* b = reinterpret_cast<unsigned long long*>(best);
    unsigned int* wi = reinterpret_cast<unsigned int*>(winner);
    hipLaunchKernelGGL(obs_best_kernel<1>, grid, dim3(kBlock), 0, s, date_ns, cell, values, n_obs, (int)n_cols, val_pitch, target_ns,
                       (int)n_time, n_cells, win, b, wi);
    ATX_LAUNCH_CHECK("obs_best_per_cell (scores)");
    hipLaunchKernelGGL(obs_best_kernel<2>, grid, dim3(kBlock), 0, s, date_ns, cell, values, n_obs, (int)n_cols, val_pitch, target_ns,
                       (int)n_time, n_cells, win, b, wi);
    ATX_LAUNCH_CHECK("obs_best_per_cell (rows)");
    return ATX_OK;
}

extern "C" int atx_obs_fill_stack(const int32_t* winner, const double* values, int64_t n_obs, int32_t n_cols, int64_t val_pitch,
                                  int32_t n_time, int64_t n_cells, double* out, int64_t pitch, int layout, void* stream) {
    ATX_REQUIRE(n_obs >= 0 && n_time >= 0 && n_cells >= 0 && n_cols > 0, ATX_EINVAL, "atx_obs_fill_stack: bad sizes");
    ATX_REQUIRE(n_obs < 0x80000000ll, ATX_EINVAL, "atx_obs_fill_stack: %lld rows do not fit an int32 row index", (long long)n_obs);
    ATX_REQUIRE(layout == ATX_COLUMNS || layout == ATX_FIELDS, ATX_EINVAL, "atx_obs_fill_stack: bad layout %d", layout);
    ATX_REQUIRE(val_pitch >= n_obs, ATX_ESHAPE, "atx_obs_fill_stack: val_pitch %lld below n_obs", (long long)val_pitch);
    const int64_t n_lev = (int64_t)n_time * n_cols;
    ATX_REQUIRE(n_lev < INT32_MAX, ATX_EINVAL, "atx_obs_fill_stack: too many levels");
    if (n_lev == 0 || n_cells == 0) return ATX_OK;
    ATX_REQUIRE(pitch >= (layout == ATX_COLUMNS ? n_lev : n_cells), ATX_ESHAPE, "atx_obs_fill_stack: pitch %lld too small", (long long)pitch);
    ATX_REQUIRE(winner && out && (values || n_obs == 0), ATX_EINVAL, "atx_obs_fill_stack: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool vec_ok = pitch % 2 == 0 && aligned16(out);
    if (layout == ATX_FIELDS) {
        const int vec = vec_ok ? 2 : 1;
        const int64_t bx = ((pitch + vec - 1) / vec + kBlock - 1) / kBlock;
        ATX_REQUIRE(bx < 0x7fffffffll, ATX_EINVAL, "atx_obs_fill_stack: too many points");
        const dim3 grid((unsigned)bx, (unsigned)(n_time < 65535 ? n_time : 65535));
        if (vec_ok)
            hipLaunchKernelGGL(obs_fill_fields_kernel<2>, grid, dim3(kBlock), 0, s, winner, values, out, n_obs, (int)n_cols, val_pitch, n_cells,
                               (int)n_time, pitch);
        else
            hipLaunchKernelGGL(obs_fill_fields_kernel<1>, grid, dim3(kBlock), 0, s, winner, values, out, n_obs, (int)n_cols, val_pitch, n_cells,
                               (int)n_time, pitch);
    } else {
        const int vec = vec_ok ? 2 : 1;
        const int64_t vpr = pitch / vec, total = n_cells * vpr;
        const int64_t blocks = (total + kBlock - 1) / kBlock;
        ATX_REQUIRE(blocks < 0x7fffffffll, ATX_EINVAL, "atx_obs_fill_stack: stack too large");
        const bool small = total < (int64_t)UINT32_MAX - kBlock;  // 32-bit index arithmetic (the division by vpr)
#define ATX_OBS_LAUNCH(V_, I_)                                                                                                       \
    hipLaunchKernelGGL((obs_fill_columns_kernel<V_, I_>), dim3((unsigned)blocks), dim3(kBlock), 0, s, winner, values, out, n_obs, \
                       (int)n_cols, val_pitch, n_cells, (int)n_lev, (I_)total, (I_)vpr)
        if (vec_ok && small) ATX_OBS_LAUNCH(2, uint32_t);
        else if (vec_ok) ATX_OBS_LAUNCH(2, int64_t);
        else if (small) ATX_OBS_LAUNCH(1, uint32_t);
        else ATX_OBS_LAUNCH(1, int64_t);
#undef ATX_OBS_LAUNCH
    }
    ATX_LAUNCH_CHECK("obs_fill_stack");
    return ATX_OK;
}
