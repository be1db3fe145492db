// Row sets of an observation table: atx_obs_order_key, atx_obs_mark_first, atx_obs_take_rows.  One row per lane.
//
// The reference's sort_by filter is df.sort_values(by=columns, kind="stable") (R: filters/tabular/sort_by.py:44-51) and its
// drop_duplicates filter df.drop_duplicates(subset) (R: filters/tabular/drop_duplicates.py:49-61).  Behind both stands pandas' order and
// equality on a key column, which is not IEEE's: -0.0 and 0.0 are ONE key, every NaN (any sign, any payload) equals every other NaN and
// sorts last, NaT likewise, +-inf order as numbers, and int64 keys compare as integers (2^53 and 2^53 + 1 differ: no route through
// float64).  Here that rule is ONE int64 key per row and column (order_key), so that the sort is the library's stable radix sort of
// int64 keys, "equal" is integer equality of the keys of adjacent sorted rows (mark_first), and what either filter returns is a gather
// of every column of the table by one int64 row list (take_rows).  tests/rowset_restatement.py holds the same statement in numpy.
//
// order_key.  Floats: with b the bit pattern and m = b & INT64_MAX the magnitude, key = INT64_MAX where m is above infinity's pattern
// (NaN), else b >= 0 ? b : -m — the sign-magnitude to two's-complement map; it sends -0.0 (m = 0) to 0, which is +0.0's key, and
// leaves +inf (0x7ff0...) below the NaN key.  float32 is widened to float64 first, which is exact, so a float32 column has the keys of
// its float64 values.  Integers and bools are their own key.  Datetimes are int64 nanoseconds; NaT (INT64_MIN) goes to INT64_MAX.
// Plain integer and compare work: no library function, no rounding, no tolerance.
//
// mark_first.  keep[order[i]] = (i == 0) or some key_k[order[i]] != key_k[order[i - 1]].  After a stable sort by the key tuple the
// rows marked are pandas' first occurrences.  With `accumulate` the kernel only ever SETS keep (more than ATX_MAX_ROWSET_COLUMNS keys:
// one launch per 16, the first plain, the others accumulating); it never clears a byte another launch set.
//
// take_rows.  out[c][i] = in[c][rows[i]] for up to ATX_MAX_ROWSET_COLUMNS columns of 1, 2, 4 or 8 bytes per element, mixed freely;
// rows[i] is read ONCE per row for all of them and compared against [0, n_in) before anything is read through it: a row index outside
// writes nothing and is counted, one atomic per wave as atx_healpix_ang2pix counts.  (torch.index_select's device-side assert would
// abort the process instead.)
//
// Launch shape, as atx_healpix.hip and atx_obs_fill_heights.hip: one row per lane, 256-lane workgroups, a grid-stride loop under a
// grid cap, 64-bit row indices.  The column tables travel by value in the kernel arguments (as atx_obs_column_ops' program does):
// they are uniform over the launch, so the loop over the columns and the branch on a column's width are scalar and every read of the
// table is a scalar load.  The sorted gather is random 1 .. 8-byte accesses per lane by nature; what fusing the columns saves is the
// C - 1 further reads of `rows` and C - 1 launches.  Measured (profiles/rowset_bench.json): that is worth 19 % with
// ascending rows and LOSES 6 % to a launch per column with a random permutation of a table larger than the last-level cache.  Column
// after column, a load and its store: issuing all loads of a row before the first store (83 VGPRs) or four at a time measured no
// better overall (profiles/rowset_take_variants.json).
#include "atx_common.hpp"

namespace atx {

// Grid cap: 2048 workgroups (8 waves per SIMD on 256 CUs, as kFhGrid); beyond 2^19 rows a lane takes further rows.
constexpr int kRsGrid = 2048;
constexpr int64_t kKeyMax = INT64_MAX;  // the key of every missing value: NaN, NaT
constexpr int64_t kInfBits = 0x7ff0000000000000ll;

static unsigned rowset_grid(int64_t n) { return grid_for(n, kBlock, kRsGrid); }

__device__ __forceinline__ int64_t float_key(double x) {
    const int64_t b = __double_as_longlong(x);
    const int64_t m = b & kKeyMax;
    if (m > kInfBits) return kKeyMax;  // NaN, whatever its sign and payload
    return b >= 0 ? b : -m;            // -0.0: m = 0, the key of +0.0
}

template <int CODE>
__device__ __forceinline__ int64_t order_key_of(const void* __restrict__ column, int64_t i) {
    if constexpr (CODE == ATX_KEY_F64) return float_key(static_cast<const double*>(column)[i]);
    else if constexpr (CODE == ATX_KEY_F32) return float_key((double)static_cast<const float*>(column)[i]);  // exact
    else if constexpr (CODE == ATX_KEY_I64) return static_cast<const int64_t*>(column)[i];
    else if constexpr (CODE == ATX_KEY_I32) return static_cast<const int32_t*>(column)[i];
    else if constexpr (CODE == ATX_KEY_I16) return static_cast<const int16_t*>(column)[i];
    else if constexpr (CODE == ATX_KEY_I8) return static_cast<const int8_t*>(column)[i];
    else if constexpr (CODE == ATX_KEY_U8) return static_cast<const uint8_t*>(column)[i];
    else if constexpr (CODE == ATX_KEY_BOOL) return static_cast<const uint8_t*>(column)[i] != 0 ? 1 : 0;
    else {  // ATX_KEY_DATETIME
        const int64_t v = static_cast<const int64_t*>(column)[i];
        return v == INT64_MIN ? kKeyMax : v;
    }
}

template <int CODE>
__global__ void __launch_bounds__(kBlock) obs_order_key_kernel(const void* __restrict__ column, int64_t n, int64_t* __restrict__ key) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) key[i] = order_key_of<CODE>(column, i);
}

struct KeyColumns {
    const int64_t* key[ATX_MAX_ROWSET_COLUMNS];
    int32_t n_keys;
};

// keep is written at order[i] only, and order is a permutation: no two lanes write one byte.  An entry of order outside [0, n) is not
// read through and marks nothing (it cannot come from a sort of n rows; the check costs two compares).
__global__ void __launch_bounds__(kBlock)
obs_mark_first_kernel(const KeyColumns p, const int64_t* __restrict__ order, int64_t n, int accumulate, uint8_t* __restrict__ keep) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const int64_t r = order[i];
        if ((uint64_t)r >= (uint64_t)n) continue;
        bool first = i == 0;
        if (!first) {
            const int64_t q = order[i - 1];
            if ((uint64_t)q >= (uint64_t)n) continue;
            for (int k = 0; k < ATX_MAX_ROWSET_COLUMNS; ++k) {
                if (k >= p.n_keys) break;
                first = first || (p.key[k][r] != p.key[k][q]);
            }
        }
        if (!accumulate) keep[r] = first ? 1 : 0;
        else if (first) keep[r] = 1;
    }
}

struct TakeColumns {
    const void* in[ATX_MAX_ROWSET_COLUMNS];
    void* out[ATX_MAX_ROWSET_COLUMNS];
    int32_t width[ATX_MAX_ROWSET_COLUMNS];  // dwords: a scalar load can fetch them at a run-time index
    int32_t n_cols;
};

// No __restrict__ on the columns: two columns of the launch may be the same input.  No output may alias an input or `rows` (the
// caller guarantees it; obs.take_rows allocates every output).
__global__ void __launch_bounds__(kBlock)
obs_take_rows_kernel(const TakeColumns p, const int64_t* __restrict__ rows, int64_t n_out, int64_t n_in, unsigned long long* n_bad) {
    unsigned long long bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_out; i += (int64_t)gridDim.x * kBlock) {
        const int64_t r = rows[i];
        if ((uint64_t)r >= (uint64_t)n_in) {  // negative or >= n_in: nothing is read through it, nothing written for the row
            bad += 1;
            continue;
        }
        for (int c = 0; c < ATX_MAX_ROWSET_COLUMNS; ++c) {
            if (c >= p.n_cols) break;
            const int w = p.width[c];
            if (w == 8) static_cast<uint64_t*>(p.out[c])[i] = static_cast<const uint64_t*>(p.in[c])[r];
            else if (w == 4) static_cast<uint32_t*>(p.out[c])[i] = static_cast<const uint32_t*>(p.in[c])[r];
            else if (w == 2) static_cast<uint16_t*>(p.out[c])[i] = static_cast<const uint16_t*>(p.in[c])[r];
            else static_cast<uint8_t*>(p.out[c])[i] = static_cast<const uint8_t*>(p.in[c])[r];
        }
    }
    // wavefront (64-lane) shuffle reduction, then one atomic per wave
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) bad += __shfl_down(bad, off, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0 && bad) atomicAdd(n_bad, bad);
}

template <int CODE>
static void launch_order_key(const void* column, int64_t n, int64_t* key, hipStream_t s) {
    hipLaunchKernelGGL(obs_order_key_kernel<CODE>, dim3(rowset_grid(n)), dim3(kBlock), 0, s, column, n, key);
}

}  // namespace atx

using namespace atx;

extern "C" int atx_obs_order_key(const void* column, int64_t n, int dtype, int64_t* key, void* stream) {
    ATX_REQUIRE(n >= 0, ATX_EINVAL, "atx_obs_order_key: %lld rows", (long long)n);
    ATX_REQUIRE(dtype >= ATX_KEY_F64 && dtype <= ATX_KEY_DATETIME, ATX_EINVAL, "atx_obs_order_key: key dtype %d (an atx_key_dtype, 0 .. 8)", dtype);
    if (n == 0) return ATX_OK;
    ATX_REQUIRE(column && key, ATX_EINVAL, "atx_obs_order_key: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (dtype) {
        case ATX_KEY_F64: launch_order_key<ATX_KEY_F64>(column, n, key, s); break;
        case ATX_KEY_F32: launch_order_key<ATX_KEY_F32>(column, n, key, s); break;
        case ATX_KEY_I64: launch_order_key<ATX_KEY_I64>(column, n, key, s); break;
        case ATX_KEY_I32: launch_order_key<ATX_KEY_I32>(column, n, key, s); break;
        case ATX_KEY_I16: launch_order_key<ATX_KEY_I16>(column, n, key, s); break;
        case ATX_KEY_I8: launch_order_key<ATX_KEY_I8>(column, n, key, s); break;
        case ATX_KEY_U8: launch_order_key<ATX_KEY_U8>(column, n, key, s); break;
        case ATX_KEY_BOOL: launch_order_key<ATX_KEY_BOOL>(column, n, key, s); break;
        default: launch_order_key<ATX_KEY_DATETIME>(column, n, key, s); break;
    }
    ATX_LAUNCH_CHECK("obs_order_key");
    return ATX_OK;
}

extern "C" int atx_obs_mark_first(int32_t n_keys, const int64_t* const* keys, const int64_t* order, int64_t n, int accumulate, uint8_t* keep,
                                  void* stream) {
    ATX_REQUIRE(n >= 0, ATX_EINVAL, "atx_obs_mark_first: %lld rows", (long long)n);
    ATX_REQUIRE(n_keys >= 1 && n_keys <= ATX_MAX_ROWSET_COLUMNS, ATX_EINVAL, "atx_obs_mark_first: 1 .. %d key columns, got %d",
                ATX_MAX_ROWSET_COLUMNS, (int)n_keys);
    ATX_REQUIRE(accumulate == 0 || accumulate == 1, ATX_EINVAL, "atx_obs_mark_first: accumulate %d (0 or 1)", accumulate);
    ATX_REQUIRE(keys, ATX_EINVAL, "atx_obs_mark_first: null key table");
    KeyColumns p = {};
    p.n_keys = n_keys;
    for (int k = 0; k < n_keys; ++k) {
        ATX_REQUIRE(keys[k] || n == 0, ATX_EINVAL, "atx_obs_mark_first: key column %d is null", k);
        p.key[k] = keys[k];
    }
    if (n == 0) return ATX_OK;
    ATX_REQUIRE(order && keep, ATX_EINVAL, "atx_obs_mark_first: null pointer");
    hipLaunchKernelGGL(obs_mark_first_kernel, dim3(rowset_grid(n)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), p, order, n, accumulate, keep);
    ATX_LAUNCH_CHECK("obs_mark_first");
    return ATX_OK;
}

extern "C" int atx_obs_take_rows(int32_t n_cols, const void* const* in, void* const* out, const int32_t* width, const int64_t* rows,
                                 int64_t n_out, int64_t n_in, int64_t* n_bad, void* stream) {
    ATX_REQUIRE(n_out >= 0 && n_in >= 0, ATX_EINVAL, "atx_obs_take_rows: %lld rows out of %lld", (long long)n_out, (long long)n_in);
    ATX_REQUIRE(n_cols >= 1 && n_cols <= ATX_MAX_ROWSET_COLUMNS, ATX_EINVAL, "atx_obs_take_rows: 1 .. %d columns, got %d", ATX_MAX_ROWSET_COLUMNS,
                (int)n_cols);
    ATX_REQUIRE(in && out && width, ATX_EINVAL, "atx_obs_take_rows: null column table");
    ATX_REQUIRE(n_bad, ATX_EINVAL, "atx_obs_take_rows: null n_bad");
    TakeColumns p = {};
    p.n_cols = n_cols;
    for (int c = 0; c < n_cols; ++c) {
        ATX_REQUIRE(width[c] == 1 || width[c] == 2 || width[c] == 4 || width[c] == 8, ATX_EINVAL,
                    "atx_obs_take_rows: column %d has elements of %d bytes (1, 2, 4 or 8)", c, (int)width[c]);
        ATX_REQUIRE(out[c] || n_out == 0, ATX_EINVAL, "atx_obs_take_rows: output column %d is null", c);
        ATX_REQUIRE(in[c] || n_in == 0 || n_out == 0, ATX_EINVAL, "atx_obs_take_rows: input column %d is null", c);
        p.in[c] = in[c];
        p.out[c] = out[c];
        p.width[c] = width[c];
    }
    ATX_REQUIRE(rows || n_out == 0, ATX_EINVAL, "atx_obs_take_rows: null rows");
    if (n_out == 0) return ATX_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int st = hip_status(hipMemsetAsync(n_bad, 0, sizeof(int64_t), s), "atx_obs_take_rows memset");
    if (st != ATX_OK) return st;
    hipLaunchKernelGGL(obs_take_rows_kernel, dim3(rowset_grid(n_out)), dim3(kBlock), 0, s, p, rows, n_out, n_in,
                       reinterpret_cast<unsigned long long*>(n_bad));
    ATX_LAUNCH_CHECK("obs_take_rows");
    return ATX_OK;
}
