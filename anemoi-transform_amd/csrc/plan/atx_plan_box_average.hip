// Grid-box-average weights between two row-structured grids, built in HBM: atx_plan_box_average_count / _fill (include/atx_plan.h).
//
// interp.box_average_rows(device=False) is the statement; tests/box_average_restatement.py holds it again as plain loops.  After the
// host's sin() of the latitude edges only min, max, -, *, / and integer arithmetic remain, and the build has no contraction
// (-ffp-contract=off), so what these kernels write equals the host statement bit for bit (tests/test_gpu_box_average.py).
//
// One target cell per lane.  The lane finds its row by binary search in the target row starts and the band of source rows whose
// latitude range meets its own by two binary searches in zs; a source row of the band takes part iff it passes the dz rule.  Within
// a source row of ns cells, target cell i of nt meets the cells jlo .. jhi (unwrapped, possibly negative or >= ns), where in units of
// 360 / (2 ns nt) degrees the target arc is [a, b) = [(2i-1) ns, (2i+1) ns) and source cell j is [(2j-1) nt, (2j+1) nt):
//     jlo = floor((a - nt) / (2 nt)) + 1      the first j with (2j+1) nt > a
//     jhi = floor((b + nt - 1) / (2 nt))      the last  j with (2j-1) nt < b
// ns, nt >= 2 gives 2 ns + 2 nt <= 2 ns nt: the two arcs cannot meet at both ends, so the run has at most ns cells and j mod ns names
// each once.  `count` adds jhi - jlo + 1 over the band; `fill` walks the run in ascending j mod ns (the part that wrapped to j = 0 ...
// first), once to accumulate tot from 0 in the order of the entries and once more to write index and raw / tot — the weights are
// recomputed, not read back, so a lane never reads what it wrote.
//
// Launch shape, as atx_text_statid.hip / atx_obs_rowset.hip: 256-lane workgroups, a grid-stride loop under a grid cap, 64-bit target
// counters.  No atomics, no LDS, no scratch (profiles/box_average_resources.json); plain vector stores.  The row tables are validated
// by the caller before upload; whatever they hold, every read stays inside the tables as sized by the arguments, and `fill` writes
// only inside [indptr[t], min(indptr[t+1], nnz)).
#include "../../../include/atx_plan.h"
#include "../atx_host.hpp"

namespace atx_plan {

constexpr int kBlock = 256;  // 4 waves: one per SIMD of a CU
constexpr int kGrid = 2048;  // grid cap, as kRsGrid: beyond 2^19 targets a lane takes further targets

struct RowTable {
    const double* __restrict__ z;       // [rows + 1]
    const int64_t* __restrict__ len;    // [rows]
    const int64_t* __restrict__ start;  // [rows + 1]
    int64_t rows;
};

__host__ __device__ __forceinline__ int64_t floor_div(int64_t a, int64_t b) {  // b > 0
    const int64_t q = a / b;
    return (a % b < 0) ? q - 1 : q;
}

// One source row's share of a target cell: the latitude overlap and the cyclic run of cells.
struct Run {
    int64_t q, ns, a, b, jlo, count;
    double dz;
};

// Calls f(run) for every source row that takes part in target t, north to south.
template <class F>
__host__ __device__ __forceinline__ void for_each_run(const RowTable& src, const RowTable& tgt, int64_t t, int64_t& nt_out, F&& f) {
    int64_t lo = 0, hi = tgt.rows;  // start[lo] <= t < start[hi]
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (tgt.start[mid] <= t) lo = mid;
        else hi = mid;
    }
    const int64_t r = lo, i = t - tgt.start[r], nt = tgt.len[r];
    nt_out = nt;
    if (nt < 2 || i < 0 || i >= nt) return;  // a table the caller should have refused
    const double top = tgt.z[r], bot = tgt.z[r + 1];
    const double threshold = 0x1p-40 * (top - bot);

    lo = 0, hi = src.rows;  // the first row whose lower edge lies below `top`
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (src.z[mid + 1] < top) hi = mid;
        else lo = mid + 1;
    }
    const int64_t q0 = lo;
    hi = src.rows;  // the first row at or after q0 whose upper edge does not lie above `bot`
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (src.z[mid] <= bot) hi = mid;
        else lo = mid + 1;
    }
    const int64_t q1 = lo;

    for (int64_t q = q0; q < q1; ++q) {
        const double zn = src.z[q], zl = src.z[q + 1];
        const double dz = (top < zn ? top : zn) - (bot > zl ? bot : zl);
        if (!(dz > threshold)) continue;
        const int64_t ns = src.len[q];
        if (ns < 2) continue;
        Run run;
        run.q = q;
        run.ns = ns;
        run.dz = dz;
        run.a = (2 * i - 1) * ns;
        run.b = (2 * i + 1) * ns;
        run.jlo = floor_div(run.a - nt, 2 * nt) + 1;
        run.count = (run.b + nt - 1) / (2 * nt) - run.jlo + 1;
        f(run);
    }
}

__global__ __launch_bounds__(kBlock) void box_average_count_kernel(RowTable src, RowTable tgt, int64_t n_tgt, int64_t* __restrict__ count) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < n_tgt; t += stride) {
        int64_t total = 0, nt;
        for_each_run(src, tgt, t, nt, [&](const Run& run) { total += run.count; });
        count[t] = total;
    }
}

// Calls f(source index, raw weight) for the entries of one run in ascending source index.
template <class F>
__host__ __device__ __forceinline__ void for_each_entry(const RowTable& src, const Run& run, int64_t nt, F&& f) {
    const int64_t ns = run.ns, first = src.start[run.q];
    int64_t s = run.jlo % ns;
    if (s < 0) s += ns;
    const int64_t wrapped = s + run.count > ns ? s + run.count - ns : 0;  // entries that fall on j = 0 ...: they come first
    const double units = (double)(2 * ns * nt);
    for (int64_t m = 0; m < run.count; ++m) {
        const int64_t k = m < wrapped ? run.count - wrapped + m : m - wrapped;  // position along the unwrapped run
        const int64_t ju = run.jlo + k;
        const int64_t east = (2 * ju + 1) * nt, west = (2 * ju - 1) * nt;
        const int64_t ov = (run.b < east ? run.b : east) - (run.a > west ? run.a : west);
        const int64_t j = m < wrapped ? m : s + k;
        f(first + j, run.dz * ((double)ov / units));
    }
}

__global__ __launch_bounds__(kBlock) void box_average_fill_kernel(RowTable src, RowTable tgt, int64_t n_tgt,
                                                                  const int32_t* __restrict__ indptr, int64_t nnz,
                                                                  int32_t* __restrict__ indices, double* __restrict__ data) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < n_tgt; t += stride) {
        int64_t nt;
        double tot = 0.0;
        for_each_run(src, tgt, t, nt, [&](const Run& run) { for_each_entry(src, run, nt, [&](int64_t, double raw) { tot += raw; }); });
        int64_t p = indptr[t], end = indptr[t + 1];
        if (end > nnz) end = nnz;
        if (p < 0) continue;
        for_each_run(src, tgt, t, nt, [&](const Run& run) {
            for_each_entry(src, run, nt, [&](int64_t column, double raw) {
                if (p < end) {
                    indices[p] = (int32_t)column;
                    data[p] = raw / tot;
                }
                ++p;
            });
        });
    }
}

static int check(const char* fn, const void* zs, const void* src_len, const void* src_start, int64_t n_src_rows, int64_t n_src,
                 const void* zt, const void* tgt_len, const void* tgt_start, int64_t n_tgt_rows, int64_t n_tgt) {
    constexpr int64_t kMax = 2147483647;
    ATX_REQUIRE(n_src_rows >= 1 && n_src_rows <= kMax && n_tgt_rows >= 1 && n_tgt_rows <= kMax, ATX_EINVAL,
                "%s: n_src_rows = %lld, n_tgt_rows = %lld: the number of rows is outside 1 .. 2^31 - 1", fn, (long long)n_src_rows,
                (long long)n_tgt_rows);
    ATX_REQUIRE(n_src >= 1 && n_src <= kMax, ATX_EINVAL, "%s: n_src = %lld is outside 1 .. 2^31 - 1", fn, (long long)n_src);
    ATX_REQUIRE(n_tgt >= 0, ATX_EINVAL, "%s: n_tgt = %lld is negative", fn, (long long)n_tgt);
    ATX_REQUIRE(n_tgt == 0 || (zs && src_len && src_start && zt && tgt_len && tgt_start), ATX_EINVAL,
                "%s: null pointer in a row table (zs=%p src_len=%p src_start=%p zt=%p tgt_len=%p tgt_start=%p)", fn, zs, src_len, src_start, zt,
                tgt_len, tgt_start);
    return ATX_OK;
}

}  // namespace atx_plan

extern "C" int atx_plan_version(void) { return ATX_PLAN_VERSION; }

extern "C" const char* atx_plan_last_error(void) { return atx::last_error().c_str(); }

extern "C" int atx_plan_box_average_count(const double* zs, const int64_t* src_len, const int64_t* src_start, int64_t n_src_rows,
                                          int64_t n_src, const double* zt, const int64_t* tgt_len, const int64_t* tgt_start,
                                          int64_t n_tgt_rows, int64_t n_tgt, int64_t* count, void* stream) {
    using namespace atx_plan;
    const char* fn = "atx_plan_box_average_count";
    const int st = check(fn, zs, src_len, src_start, n_src_rows, n_src, zt, tgt_len, tgt_start, n_tgt_rows, n_tgt);
    if (st != ATX_OK) return st;
    if (n_tgt == 0) return ATX_OK;
    ATX_REQUIRE(count, ATX_EINVAL, "%s: null pointer (count) with n_tgt = %lld", fn, (long long)n_tgt);
    const RowTable src{zs, src_len, src_start, n_src_rows}, tgt{zt, tgt_len, tgt_start, n_tgt_rows};
    hipLaunchKernelGGL(box_average_count_kernel, dim3(atx::grid_for(n_tgt, kBlock, kGrid)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), src,
                       tgt, n_tgt, count);
    ATX_LAUNCH_CHECK(fn);
    return ATX_OK;
}

extern "C" int atx_plan_box_average_fill(const double* zs, const int64_t* src_len, const int64_t* src_start, int64_t n_src_rows,
                                         int64_t n_src, const double* zt, const int64_t* tgt_len, const int64_t* tgt_start,
                                         int64_t n_tgt_rows, int64_t n_tgt, const int32_t* indptr, int64_t nnz, int32_t* indices,
                                         double* data, void* stream) {
    using namespace atx_plan;
    const char* fn = "atx_plan_box_average_fill";
    const int st = check(fn, zs, src_len, src_start, n_src_rows, n_src, zt, tgt_len, tgt_start, n_tgt_rows, n_tgt);
    if (st != ATX_OK) return st;
    ATX_REQUIRE(nnz >= 0 && nnz <= 2147483647, ATX_EINVAL, "%s: nnz = %lld is outside 0 .. 2^31 - 1", fn, (long long)nnz);
    if (n_tgt == 0) return ATX_OK;
    ATX_REQUIRE(indptr && (nnz == 0 || (indices && data)), ATX_EINVAL, "%s: null pointer (indptr=%p indices=%p data=%p) with n_tgt = %lld, nnz = %lld",
                fn, (const void*)indptr, (void*)indices, (void*)data, (long long)n_tgt, (long long)nnz);
    const RowTable src{zs, src_len, src_start, n_src_rows}, tgt{zt, tgt_len, tgt_start, n_tgt_rows};
    hipLaunchKernelGGL(box_average_fill_kernel, dim3(atx::grid_for(n_tgt, kBlock, kGrid)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), src,
                       tgt, n_tgt, indptr, nnz, indices, data);
    ATX_LAUNCH_CHECK(fn);
    return ATX_OK;
}
