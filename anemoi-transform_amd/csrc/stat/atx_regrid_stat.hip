// Grid-box statistics: atx_regrid_csr_stat (include/atx_stat.h holds the statement), built into a library of its own,
// lib/libatx_stat.so — libatx's entry points are a fixed, tested set, as for libatx_plan / _mesh / _text / _missing.
//
// The rows of a CSR matrix name the source cells under each target; where every gather of libatx and libatx_missing computes a
// weighted sum over them, these kernels take the maximum, the minimum, the class with the largest weight (mode) or the weighted
// variance / standard deviation.  Column stacks only, natural target order, no level program.  The device helpers (Pack, store_out,
// load_src, xcd_tile, quiet_nan) and cols_vector_ok are libatx's own headers, included, not copied; nothing of libatx is linked: the
// message cell (atx_host.hpp), the stack check and the ATX_VALIDATE range check (atx_regrid_check.hpp) are the same source,
// compiled into this library.
//
// One (target, vector) item per lane, consecutive lanes on consecutive vectors of a column, as the kernels of
// missing/atx_regrid_missing.hip: the lane reads its row's index and weight words itself, kStatStep entries at a time with their source
// vectors in flight together, and stores once.  Per lane, whatever the statistic (StatRow): tot and the running largest weight per row;
// den and three bits (a missing source seen, a valid one seen, the heaviest entry so far was missing) per element.  On top of that
//   MAXIMUM / MINIMUM  one walk, the running extreme per element; without weights (data == NULL) no weight word is read;
//   VARIANCE / STDDEV  two walks: num in the first, then mean = num / den, and s in the second, whose source vectors hit L2;
//   MODE               one walk with a table of kModeClasses (value, running weight) pairs per element, a new value appended in row
//                      order, so every class adds its weights in the statement's order; an element that meets more distinct values
//                      sets its overflow bit and the lane redoes its vector by the quadratic walk of the statement.
// No LDS, no barrier, no scratch (every private array is indexed by unrolled constants; profiles/stat_resources.json).
#include "../../../include/atx_stat.h"
#include "../atx_common.hpp"
#include "../atx_regrid_check.hpp"
#include "../atx_regrid_decl.hpp"

namespace atx {

constexpr int kStatBlock = 256;   // lanes per workgroup, the direct kernel's
constexpr int kStatStep = 4;      // entries of a row whose source vectors are in flight together
constexpr int kModeClasses = 8;   // distinct values per element that MODE keeps in registers; more: the quadratic walk

// What the kernels are instantiated for: the two extremes, mode, and variance (the standard deviation is its square root).
enum StatKind { kMax = 0, kMin = 1, kMode = 2, kVar = 3 };

// The entries of one row, kStatStep at a time: f(w, v) for each in table order.  The slots past the row's end load entry j0 again
// (an address the lane reads anyway) and are not handed on.
template <typename T, int VEC, bool WEIGHTED, typename F>
__device__ __forceinline__ void stat_walk(const T* __restrict__ src, const int32_t* __restrict__ ip, const T* __restrict__ wp, int n,
                                          int64_t src_pitch, int c, F&& f) {
    using V = Pack<T, VEC>;
    for (int j0 = 0; j0 < n; j0 += kStatStep) {
        int32_t p[kStatStep];
        T wv[kStatStep];
#pragma unroll
        for (int u = 0; u < kStatStep; ++u) {
            const int j = j0 + u < n ? j0 + u : j0;
            p[u] = ip[j];
            if constexpr (WEIGHTED)
                wv[u] = wp[j];
            else
                wv[u] = T(1);
        }
        V v[kStatStep];
#pragma unroll
        for (int u = 0; u < kStatStep; ++u) v[u] = load_src<T, VEC>(src + (int64_t)p[u] * src_pitch + (int64_t)c * VEC);
#pragma unroll
        for (int u = 0; u < kStatStep; ++u) {
            if (j0 + u < n) f(wv[u], v[u]);
        }
    }
}

// What every statistic keeps of a row: the policy's inputs.
template <typename T, int VEC>
struct StatRow {
    T den[VEC];
    T tot, best;
    unsigned missing, valid, heaviest_missing;  // bit e: element e of the vector
    bool have;                                  // an entry was seen (best holds its weight)
};

template <typename T, int VEC>
__device__ __forceinline__ void stat_init(StatRow<T, VEC>& a) {
#pragma unroll
    for (int e = 0; e < VEC; ++e) a.den[e] = T(0);
    a.tot = a.best = T(0);
    a.missing = a.valid = a.heaviest_missing = 0u;
    a.have = false;
}

// One entry: weight w, source vector v.  Returns the bits of the elements whose source is a number.
template <typename T, int VEC>
__device__ __forceinline__ unsigned stat_entry(StatRow<T, VEC>& a, T w, const Pack<T, VEC>& v) {
    a.tot = a.tot + w;
    const bool heavier = !a.have || w > a.best;  // strict: the first among equals stays
    a.best = heavier ? w : a.best;
    a.have = true;
    unsigned numbers = 0u;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        const T x = v.v[e];
        const bool nan = x != x;
        const unsigned bit = 1u << e;
        a.den[e] = nan ? a.den[e] : a.den[e] + w;
        a.missing |= nan ? bit : 0u;
        numbers |= nan ? 0u : bit;
        if (heavier) a.heaviest_missing = (a.heaviest_missing & ~bit) | (nan ? bit : 0u);
    }
    a.valid |= numbers;
    return numbers;
}

// The elements the policy makes NaN.
template <typename T, int VEC>
__device__ __forceinline__ unsigned stat_gone(const StatRow<T, VEC>& a, int policy, T min_valid) {
    const T need = min_valid * a.tot;
    unsigned gone = ~a.valid;
    if (policy == ATX_STAT_MISSING_ANY) gone |= a.missing;
    if (policy == ATX_STAT_MISSING_HEAVIEST) gone |= a.heaviest_missing;
#pragma unroll
    for (int e = 0; e < VEC; ++e) gone |= a.den[e] < need ? 1u << e : 0u;
    return gone;
}

template <typename T, int VEC>
__device__ __forceinline__ Pack<T, VEC> stat_finish(const StatRow<T, VEC>& a, int policy, T min_valid, const Pack<T, VEC>& value) {
    const unsigned gone = stat_gone(a, policy, min_valid);
    Pack<T, VEC> r;
#pragma unroll
    for (int e = 0; e < VEC; ++e) r.v[e] = (gone >> e & 1u) ? quiet_nan<T>() : value.v[e];
    return r;
}

// sqrt, correctly rounded.  float goes through double: the double root of a float, rounded to float, is the correctly rounded float
// root (53 >= 2 * 24 + 2 bits).
__device__ __forceinline__ double stat_sqrt(double x) { return sqrt(x); }
__device__ __forceinline__ float stat_sqrt(float x) { return (float)sqrt((double)x); }

// ---- maximum / minimum ---------------------------------------------------------------------------------------------------------------
template <typename T, int VEC, bool IS_MAX, bool WEIGHTED>
__device__ __forceinline__ Pack<T, VEC> extreme_row(const T* __restrict__ src, const int32_t* __restrict__ ip, const T* __restrict__ wp, int n,
                                                    int64_t src_pitch, int c, int policy, T min_valid) {
    StatRow<T, VEC> a;
    stat_init(a);
    Pack<T, VEC> m;
#pragma unroll
    for (int e = 0; e < VEC; ++e) m.v[e] = T(0);
    stat_walk<T, VEC, WEIGHTED>(src, ip, wp, n, src_pitch, c, [&](T w, const Pack<T, VEC>& v) {
        const unsigned before = a.valid;
        const unsigned numbers = stat_entry(a, w, v);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const T x = v.v[e];
            const bool first = !(before >> e & 1u);
            const bool beyond = IS_MAX ? x > m.v[e] : x < m.v[e];
            m.v[e] = (numbers >> e & 1u) && (first || beyond) ? x : m.v[e];
        }
    });
    return stat_finish(a, policy, min_valid, m);
}

// ---- variance / standard deviation ---------------------------------------------------------------------------------------------------
template <typename T, int VEC>
__device__ __forceinline__ Pack<T, VEC> variance_row(const T* __restrict__ src, const int32_t* __restrict__ ip, const T* __restrict__ wp, int n,
                                                     int64_t src_pitch, int c, int policy, T min_valid, bool root) {
    StatRow<T, VEC> a;
    stat_init(a);
    T num[VEC], mean[VEC], s[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) num[e] = s[e] = T(0);
    stat_walk<T, VEC, true>(src, ip, wp, n, src_pitch, c, [&](T w, const Pack<T, VEC>& v) {
        const unsigned numbers = stat_entry(a, w, v);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const T prod = w * v.v[e];  // (-ffp-contract=off: a multiply and an add)
            num[e] = (numbers >> e & 1u) ? num[e] + prod : num[e];
        }
    });
#pragma unroll
    for (int e = 0; e < VEC; ++e) mean[e] = num[e] / a.den[e];  // IEEE division
    stat_walk<T, VEC, true>(src, ip, wp, n, src_pitch, c, [&](T w, const Pack<T, VEC>& v) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const T x = v.v[e];
            const T d = x - mean[e];
            const T sq = d * d;
            const T prod = w * sq;
            s[e] = x != x ? s[e] : s[e] + prod;
        }
    });
    Pack<T, VEC> r;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        const T var = s[e] / a.den[e];
        r.v[e] = root ? stat_sqrt(var) : var;
    }
    return stat_finish(a, policy, min_valid, r);
}

// ---- mode ----------------------------------------------------------------------------------------------------------------------------
// The statement as it is written, for the lane's whole vector: every valid entry j against the best so far, W_j by a walk of its own.
template <typename T, int VEC>
__device__ __forceinline__ Pack<T, VEC> mode_quadratic(const T* __restrict__ src, const int32_t* __restrict__ ip, const T* __restrict__ wp, int n,
                                                       int64_t src_pitch, int c) {
    using V = Pack<T, VEC>;
    V bx;
    T bw[VEC];
    unsigned have = 0u;
#pragma unroll
    for (int e = 0; e < VEC; ++e) bx.v[e] = bw[e] = T(0);
    for (int j = 0; j < n; ++j) {
        const V xj = load_src<T, VEC>(src + (int64_t)ip[j] * src_pitch + (int64_t)c * VEC);
        T wj[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) wj[e] = T(0);
        stat_walk<T, VEC, true>(src, ip, wp, n, src_pitch, c, [&](T w, const V& v) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) wj[e] = v.v[e] == xj.v[e] ? wj[e] + w : wj[e];  // (a NaN equals nothing)
        });
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const T x = xj.v[e];
            const bool number = x == x;
            const bool first = !(have >> e & 1u);
            const bool better = wj[e] > bw[e] || (wj[e] == bw[e] && x < bx.v[e]);
            const bool take = number && (first || better);
            bx.v[e] = take ? x : bx.v[e];
            bw[e] = take ? wj[e] : bw[e];
            have |= number ? 1u << e : 0u;
        }
    }
    return bx;
}

template <typename T, int VEC>
__device__ __forceinline__ Pack<T, VEC> mode_row(const T* __restrict__ src, const int32_t* __restrict__ ip, const T* __restrict__ wp, int n,
                                                 int64_t src_pitch, int c, int policy, T min_valid) {
    using V = Pack<T, VEC>;
    StatRow<T, VEC> a;
    stat_init(a);
    T val[VEC][kModeClasses], wgt[VEC][kModeClasses];  // the classes of element e in the order they were met; an empty slot holds NaN
    int count[VEC];
    unsigned overflow = 0u;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        count[e] = 0;
#pragma unroll
        for (int k = 0; k < kModeClasses; ++k) {
            val[e][k] = quiet_nan<T>();
            wgt[e][k] = T(0);
        }
    }
    stat_walk<T, VEC, true>(src, ip, wp, n, src_pitch, c, [&](T w, const V& v) {
        const unsigned numbers = stat_entry(a, w, v);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const T x = v.v[e];
            bool found = false;
#pragma unroll
            for (int k = 0; k < kModeClasses; ++k) {
                const bool hit = val[e][k] == x;  // (false for an empty slot and for a NaN source)
                wgt[e][k] = hit ? wgt[e][k] + w : wgt[e][k];
                found = found || hit;
            }
            const bool fresh = (numbers >> e & 1u) && !found;
            overflow |= fresh && count[e] == kModeClasses ? 1u << e : 0u;
#pragma unroll
            for (int k = 0; k < kModeClasses; ++k) {
                const bool put = fresh && count[e] == k;
                val[e][k] = put ? x : val[e][k];
                wgt[e][k] = put ? T(0) + w : wgt[e][k];
            }
            count[e] += fresh && count[e] < kModeClasses ? 1 : 0;
        }
    });
    V r;
    if (overflow != 0u) {
        r = mode_quadratic<T, VEC>(src, ip, wp, n, src_pitch, c);
    } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            T bx = val[e][0], bw = wgt[e][0];
#pragma unroll
            for (int k = 1; k < kModeClasses; ++k) {
                const bool take = k < count[e] && (wgt[e][k] > bw || (wgt[e][k] == bw && val[e][k] < bx));
                bx = take ? val[e][k] : bx;
                bw = take ? wgt[e][k] : bw;
            }
            r.v[e] = bx;
        }
    }
    return stat_finish(a, policy, min_valid, r);
}

// ---- the kernel ----------------------------------------------------------------------------------------------------------------------
template <typename T, int VEC, int KIND, bool WEIGHTED>
__global__ void __launch_bounds__(kStatBlock)
regrid_cols_csr_stat_kernel(const T* __restrict__ src, T* __restrict__ out, const int32_t* __restrict__ indptr,
                            const int32_t* __restrict__ indices, const T* __restrict__ data, int64_t n_items, int C, int64_t src_pitch,
                            int64_t out_pitch, unsigned n_blocks, int policy, T min_valid, int root) {
    using V = Pack<T, VEC>;
    const unsigned b = xcd_tile(blockIdx.x, n_blocks);  // neighbouring targets meet in one XCD's L2
    const int64_t q = (int64_t)b * kStatBlock + threadIdx.x;
    if (q >= n_items) return;
    const int64_t t = q / C;
    const int c = (int)(q - t * C);
    const int64_t first = indptr[t];
    const int n = (int)(indptr[t + 1] - first);
    const int32_t* ip = indices + first;
    const T* wp = WEIGHTED ? data + first : nullptr;
    V r;
    if constexpr (KIND == kMax)
        r = extreme_row<T, VEC, true, WEIGHTED>(src, ip, wp, n, src_pitch, c, policy, min_valid);
    else if constexpr (KIND == kMin)
        r = extreme_row<T, VEC, false, WEIGHTED>(src, ip, wp, n, src_pitch, c, policy, min_valid);
    else if constexpr (KIND == kMode)
        r = mode_row<T, VEC>(src, ip, wp, n, src_pitch, c, policy, min_valid);
    else
        r = variance_row<T, VEC>(src, ip, wp, n, src_pitch, c, policy, min_valid, root != 0);
    store_out(reinterpret_cast<V*>(out + t * out_pitch + (int64_t)c * VEC), r);
}

// The vector width a column stack allows — the condition of regrid_cols_ell: 16-byte bases and pitches, the last (partial) vector
// inside both pitches; anything else runs one element per lane.
template <typename T>
static bool stat_vector_ok(const void* src, const void* out, int n_lev, int64_t sp, int64_t op) {
    constexpr int VEC = Vec16<T>::N;
    const int64_t covered = ((int64_t)(n_lev + VEC - 1) / VEC) * VEC;
    return cols_vector_ok<T>(src, out, sp, op) && covered <= sp && covered <= op;
}

template <typename T, int VEC>
static int launch_csr_stat(const T* src, T* out, const int32_t* indptr, const int32_t* indices, const T* data, int64_t n_tgt, int n_lev,
                           int64_t sp, int64_t op, int statistic, int policy, T min_valid, hipStream_t st) {
    const int C = (n_lev + VEC - 1) / VEC;
    const int64_t n_items = n_tgt * C;
    const int64_t blocks = (n_items + kStatBlock - 1) / kStatBlock;
    ATX_REQUIRE(blocks <= INT32_MAX, ATX_ENOTIMPL, "atx_regrid_csr_stat: %lld x %d items exceed one launch", (long long)n_tgt, C);
    const unsigned n_blocks = (unsigned)blocks;
    auto launch = [&](auto kind, auto weighted) -> int {
        constexpr int KIND = decltype(kind)::value;
        constexpr bool WEIGHTED = decltype(weighted)::value;
        hipLaunchKernelGGL((regrid_cols_csr_stat_kernel<T, VEC, KIND, WEIGHTED>), dim3(n_blocks), dim3(kStatBlock), 0, st, src, out, indptr, indices,
                           data, n_items, C, sp, op, n_blocks, policy, min_valid, statistic == ATX_STAT_STDDEV ? 1 : 0);
        ATX_LAUNCH_CHECK("regrid_cols_csr_stat");
        return ATX_OK;
    };
    switch (statistic) {
        case ATX_STAT_MAXIMUM: return data ? launch(IntTag<kMax>{}, std::true_type{}) : launch(IntTag<kMax>{}, std::false_type{});
        case ATX_STAT_MINIMUM: return data ? launch(IntTag<kMin>{}, std::true_type{}) : launch(IntTag<kMin>{}, std::false_type{});
        case ATX_STAT_MODE: return launch(IntTag<kMode>{}, std::true_type{});
        default: return launch(IntTag<kVar>{}, std::true_type{});
    }
}

template <typename T>
static int regrid_csr_stat_typed(const void* src_, void* out_, const int32_t* indptr, const int32_t* indices, const void* data_, int64_t n_tgt,
                                 int n_lev, int64_t sp, int64_t op, int statistic, int policy, double min_valid, hipStream_t st) {
    const T* src = static_cast<const T*>(src_);
    T* out = static_cast<T*>(out_);
    const T* data = static_cast<const T*>(data_);
    if (stat_vector_ok<T>(src_, out_, n_lev, sp, op))
        return launch_csr_stat<T, Vec16<T>::N>(src, out, indptr, indices, data, n_tgt, n_lev, sp, op, statistic, policy, static_cast<T>(min_valid), st);
    return launch_csr_stat<T, 1>(src, out, indptr, indices, data, n_tgt, n_lev, sp, op, statistic, policy, static_cast<T>(min_valid), st);
}

}  // namespace atx

using namespace atx;

extern "C" int atx_stat_version(void) { return ATX_STAT_VERSION; }

extern "C" const char* atx_stat_last_error(void) { return last_error().c_str(); }

extern "C" int atx_regrid_csr_stat(const void* src, void* out, const int32_t* indptr, const int32_t* indices, const void* data, int64_t n_src,
                                   int64_t n_tgt, int64_t nnz, int64_t n_lev, int64_t src_pitch, int64_t out_pitch, int dtype, int layout,
                                   int statistic, int policy, double min_valid, void* stream) {
    const char* fn = "atx_regrid_csr_stat";
    int st = check_stack_args(fn, src, out, n_src, n_tgt, n_lev, src_pitch, out_pitch, dtype, layout);
    if (st != ATX_OK) return st;
    ATX_REQUIRE(indptr || n_tgt == 0, ATX_EINVAL, "%s: null indptr", fn);
    ATX_REQUIRE(nnz >= 0 && nnz <= INT32_MAX, ATX_ENOTIMPL, "%s: nnz=%lld outside int32", fn, (long long)nnz);
    ATX_REQUIRE(nnz == 0 || indices, ATX_EINVAL, "%s: null indices", fn);
    ATX_REQUIRE(statistic >= ATX_STAT_MAXIMUM && statistic <= ATX_STAT_STDDEV, ATX_EINVAL, "%s: unknown statistic %d", fn, statistic);
    ATX_REQUIRE(policy >= ATX_STAT_MISSING_ANY && policy <= ATX_STAT_MISSING_HEAVIEST, ATX_EINVAL, "%s: unknown missing-value policy %d", fn, policy);
    ATX_REQUIRE(min_valid >= 0.0 && min_valid <= 1.0, ATX_EINVAL, "%s: min_valid = %g is outside [0, 1]", fn, min_valid);  // (NaN fails both)
    ATX_REQUIRE(data || statistic == ATX_STAT_MAXIMUM || statistic == ATX_STAT_MINIMUM, ATX_EINVAL,
                "%s: null data (only the maximum and the minimum are defined without weights)", fn);
    ATX_REQUIRE(layout == ATX_COLUMNS, ATX_ENOTIMPL, "%s: column stacks only (convert an ATX_FIELDS stack with atx_relayout)", fn);
    if (n_tgt == 0) return ATX_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (validation_on()) {
        st = validate_table(fn, "indices", indices, nnz, 0, n_src, s);
        if (st == ATX_OK) st = validate_table(fn, "indptr", indptr, n_tgt + 1, 0, nnz + 1, s);
        if (st != ATX_OK) return st;
    }
    if (dtype == ATX_F32)
        return regrid_csr_stat_typed<float>(src, out, indptr, indices, data, n_tgt, (int)n_lev, src_pitch, out_pitch, statistic, policy, min_valid, s);
    return regrid_csr_stat_typed<double>(src, out, indptr, indices, data, n_tgt, (int)n_lev, src_pitch, out_pitch, statistic, policy, min_valid, s);
}
