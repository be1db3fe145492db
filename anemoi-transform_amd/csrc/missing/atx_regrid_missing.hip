// The weighted gather with missing values: atx_regrid_ell_missing / atx_regrid_csr_missing (include/atx_missing.h holds the statement),
// built into a library of its own, lib/libatx_missing.so — libatx's entry points are a fixed, tested set, as for libatx_plan / _mesh / _text.
//
// A NaN source is dropped from its row, the remaining weights renormalise, and a policy decides when the target itself is missing —
// what MIR does where `self.matrix @ data` (R: filters/fields/regrid.py:310) makes the target NaN as soon as one of its k sources is.
// Column stacks only, natural target order, no level program: the existing gather kernels and their dispatch are untouched.  The
// device helpers (Pack, store_out, load_src, xcd_tile, quiet_nan) and cols_vector_ok are libatx's own headers, included, not copied;
// nothing of libatx is linked: the message cell (atx_host.hpp), the stack check and the ATX_VALIDATE range check
// (atx_regrid_check.hpp) are the same source, compiled into this library.
//
// One (target, vector) item per lane, consecutive lanes on consecutive vectors of a column, as the direct kernel of
// atx_regrid_columns.inc: the lane reads its row's index and weight words itself, the source vectors with plain loads, and stores once.
// The row is walked ONCE, kStep entries at a time with their source vectors in flight together:
//   tot and the running largest weight are per row; num, den and three bits (a missing source seen, a valid one seen, the heaviest entry
//   so far was missing) per element.  "The first present entry with the largest weight" needs no pass of its own — when an entry's
//   weight is strictly above every earlier one, the element's heaviest-missing bit becomes "this source is NaN", else it stays.
// Where no element of the lane's vector met a NaN the lane stores num as it is — scipy's csr_matvec loop, no division; the division and
// the policy sit behind one branch that a wave of complete data never takes.
// No LDS, no barrier, no scratch (every private array is indexed by unrolled constants; profiles/regrid_missing_resources.json).
#include "../../../include/atx_missing.h"
#include "../atx_common.hpp"
#include "../atx_regrid_check.hpp"
#include "../atx_regrid_decl.hpp"

namespace atx {

constexpr int kMissingBlock = 256;  // lanes per workgroup, the direct kernel's
constexpr int kMissingStep = 4;     // entries of a run-time row (k outside the ladder, CSR) whose source vectors are in flight together

// Per-lane state of one (target, vector) item.
template <typename T, int VEC>
struct MissingAcc {
    T num[VEC], den[VEC];
    T tot, best;
    unsigned missing, valid, heaviest_missing;  // bit e: element e of the vector
    bool have;                                  // a present entry was seen (best holds its weight)
};

template <typename T, int VEC>
__device__ __forceinline__ void missing_init(MissingAcc<T, VEC>& a) {
#pragma unroll
    for (int e = 0; e < VEC; ++e) a.num[e] = a.den[e] = T(0);
    a.tot = a.best = T(0);
    a.missing = a.valid = a.heaviest_missing = 0u;
    a.have = false;
}

// One present entry: weight w, source vector v.
template <typename T, int VEC>
__device__ __forceinline__ void missing_entry(MissingAcc<T, VEC>& a, T w, const Pack<T, VEC>& v) {
    a.tot = a.tot + w;
    const bool heavier = !a.have || w > a.best;  // strict: the first among equals stays
    a.best = heavier ? w : a.best;
    a.have = true;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        const T x = v.v[e];
        const bool nan = x != x;
        const T prod = w * x;  // (-ffp-contract=off: a multiply and an add)
        a.num[e] = nan ? a.num[e] : a.num[e] + prod;
        a.den[e] = nan ? a.den[e] : a.den[e] + w;
        const unsigned bit = 1u << e;
        a.missing |= nan ? bit : 0u;
        a.valid |= nan ? 0u : bit;
        if (heavier) a.heaviest_missing = (a.heaviest_missing & ~bit) | (nan ? bit : 0u);
    }
}

template <typename T, int VEC>
__device__ __forceinline__ Pack<T, VEC> missing_result(const MissingAcc<T, VEC>& a, bool heaviest, T min_valid) {
    Pack<T, VEC> r;
#pragma unroll
    for (int e = 0; e < VEC; ++e) r.v[e] = a.num[e];
    if (a.missing != 0u) {  // a wave of complete data skips the divisions
        const T need = min_valid * a.tot;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const unsigned bit = 1u << e;
            const bool gone = !(a.valid & bit) || (heaviest && (a.heaviest_missing & bit)) || a.den[e] < need;
            const T q = a.num[e] / a.den[e];  // IEEE division, as ATX_OP_DIV divides
            if (a.missing & bit) r.v[e] = gone ? quiet_nan<T>() : q;
        }
    }
    return r;
}

// STEP entries ip[0 .. n) / wp[0 .. n) at a time (n == STEP at compile time: the whole row in one step, every load in flight at once).
// An absent entry (negative index) and the slots past n are skipped; their loads go to the row's first source column, a line this
// lane fetches anyway (see the direct kernel).
template <typename T, int VEC, int STEP>
__device__ __forceinline__ Pack<T, VEC> missing_row(const T* __restrict__ src, const int32_t* __restrict__ ip, const T* __restrict__ wp, int n,
                                                    int64_t src_pitch, int c, bool heaviest, T min_valid) {
    using V = Pack<T, VEC>;
    MissingAcc<T, VEC> a;
    missing_init(a);
    int32_t spare = 0;
    for (int j0 = 0; j0 < n; j0 += STEP) {
        int32_t p[STEP];
        T wv[STEP];
#pragma unroll
        for (int u = 0; u < STEP; ++u) {
            const bool in = j0 + u < n;
            p[u] = in ? ip[j0 + u] : -1;
            wv[u] = in ? wp[j0 + u] : T(0);
        }
        if (j0 == 0) spare = p[0] >= 0 ? p[0] : 0;
        V v[STEP];
#pragma unroll
        for (int u = 0; u < STEP; ++u) v[u] = load_src<T, VEC>(src + (int64_t)(p[u] >= 0 ? p[u] : spare) * src_pitch + (int64_t)c * VEC);
#pragma unroll
        for (int u = 0; u < STEP; ++u) {
            if (p[u] >= 0) missing_entry(a, wv[u], v[u]);
        }
    }
    return missing_result(a, heaviest, min_valid);
}

// Fixed-k rows.  K > 0: the compile-time forms (1, 2, 3, 4, 8, 16: the whole row in flight); K == 0: any k, kMissingStep entries per step.
template <typename T, int VEC, int K>
__global__ void __launch_bounds__(kMissingBlock)
regrid_cols_ell_missing_kernel(const T* __restrict__ src, T* __restrict__ out, const int32_t* __restrict__ idx, const T* __restrict__ w,
                               int64_t n_items, int C, int k, int64_t src_pitch, int64_t out_pitch, unsigned n_blocks, int heaviest, T min_valid) {
    using V = Pack<T, VEC>;
    const unsigned b = xcd_tile(blockIdx.x, n_blocks);  // neighbouring targets meet in one XCD's L2
    const int64_t q = (int64_t)b * kMissingBlock + threadIdx.x;
    if (q >= n_items) return;
    const int64_t t = q / C;
    const int c = (int)(q - t * C);
    V r;
    if constexpr (K > 0)
        r = missing_row<T, VEC, K>(src, idx + t * K, w + t * K, K, src_pitch, c, heaviest != 0, min_valid);
    else
        r = missing_row<T, VEC, kMissingStep>(src, idx + t * k, w + t * k, k, src_pitch, c, heaviest != 0, min_valid);
    store_out(reinterpret_cast<V*>(out + t * out_pitch + (int64_t)c * VEC), r);
}

// General CSR rows: the same walk over indptr[t] .. indptr[t+1].
template <typename T, int VEC>
__global__ void __launch_bounds__(kMissingBlock)
regrid_cols_csr_missing_kernel(const T* __restrict__ src, T* __restrict__ out, const int32_t* __restrict__ indptr,
                               const int32_t* __restrict__ indices, const T* __restrict__ data, int64_t n_items, int C, int64_t src_pitch,
                               int64_t out_pitch, unsigned n_blocks, int heaviest, T min_valid) {
    using V = Pack<T, VEC>;
    const unsigned b = xcd_tile(blockIdx.x, n_blocks);
    const int64_t q = (int64_t)b * kMissingBlock + threadIdx.x;
    if (q >= n_items) return;
    const int64_t t = q / C;
    const int c = (int)(q - t * C);
    const int64_t first = indptr[t];
    const int n = (int)(indptr[t + 1] - first);
    const V r = missing_row<T, VEC, kMissingStep>(src, indices + first, data + first, n, src_pitch, c, heaviest != 0, min_valid);
    store_out(reinterpret_cast<V*>(out + t * out_pitch + (int64_t)c * VEC), r);
}

// The vector width a column stack allows — the condition of regrid_cols_ell: 16-byte bases and pitches, the last (partial) vector
// inside both pitches; anything else runs one element per lane.
template <typename T>
static bool missing_vector_ok(const void* src, const void* out, int n_lev, int64_t sp, int64_t op) {
    constexpr int VEC = Vec16<T>::N;
    const int64_t covered = ((int64_t)(n_lev + VEC - 1) / VEC) * VEC;
    return cols_vector_ok<T>(src, out, sp, op) && covered <= sp && covered <= op;
}

template <typename T, int VEC>
static int launch_ell_missing(const T* src, T* out, const int32_t* idx, const T* w, int64_t n_tgt, int k, int n_lev, int64_t sp, int64_t op,
                              bool heaviest, T min_valid, hipStream_t st) {
    const int C = (n_lev + VEC - 1) / VEC;
    const int64_t n_items = n_tgt * C;
    const int64_t blocks = (n_items + kMissingBlock - 1) / kMissingBlock;
    ATX_REQUIRE(blocks <= INT32_MAX, ATX_ENOTIMPL, "atx_regrid_ell_missing: %lld x %d items exceed one launch", (long long)n_tgt, C);
    const unsigned n_blocks = (unsigned)blocks;
    auto launch = [&](auto kc) -> int {
        constexpr int K = decltype(kc)::value;
        hipLaunchKernelGGL((regrid_cols_ell_missing_kernel<T, VEC, K>), dim3(n_blocks), dim3(kMissingBlock), 0, st, src, out, idx, w, n_items, C, k,
                           sp, op, n_blocks, heaviest ? 1 : 0, min_valid);
        ATX_LAUNCH_CHECK("regrid_cols_ell_missing");
        return ATX_OK;
    };
    // Compile-time rows where a k-NN or bilinear regrid has them (the whole row's source vectors in flight at once), the run-time loop
    // elsewhere.  O1280 -> 0.25 degree, 137 levels, k = 4 (profiles/regrid_missing_bench.json): 0.445 ms f32 / 0.836 ms f64 on the ladder —
    // the plain direct kernel's time on the same plan, 0.998 / 0.976 of it — against 0.520 / 0.967 ms for the same four sources through
    // the loop (+17 % / +16 %).  Every form is named with the k that reaches it in tests/test_gpu_regrid_missing.py.
    switch (k) {
        case 1: return launch(IntTag<1>{});
        case 2: return launch(IntTag<2>{});
        case 3: return launch(IntTag<3>{});
        case 4: return launch(IntTag<4>{});
        case 8: return launch(IntTag<8>{});
        case 16: return launch(IntTag<16>{});
        default: return launch(IntTag<0>{});
    }
}

template <typename T>
static int regrid_ell_missing_typed(const void* src_, void* out_, const int32_t* idx, const void* w_, int64_t n_tgt, int k, int n_lev, int64_t sp,
                                    int64_t op, bool heaviest, double min_valid, hipStream_t st) {
    const T* src = static_cast<const T*>(src_);
    T* out = static_cast<T*>(out_);
    const T* w = static_cast<const T*>(w_);
    if (missing_vector_ok<T>(src_, out_, n_lev, sp, op))
        return launch_ell_missing<T, Vec16<T>::N>(src, out, idx, w, n_tgt, k, n_lev, sp, op, heaviest, static_cast<T>(min_valid), st);
    return launch_ell_missing<T, 1>(src, out, idx, w, n_tgt, k, n_lev, sp, op, heaviest, static_cast<T>(min_valid), st);
}

template <typename T, int VEC>
static int launch_csr_missing(const T* src, T* out, const int32_t* indptr, const int32_t* indices, const T* data, int64_t n_tgt, int n_lev,
                              int64_t sp, int64_t op, bool heaviest, T min_valid, hipStream_t st) {
    const int C = (n_lev + VEC - 1) / VEC;
    const int64_t n_items = n_tgt * C;
    const int64_t blocks = (n_items + kMissingBlock - 1) / kMissingBlock;
    ATX_REQUIRE(blocks <= INT32_MAX, ATX_ENOTIMPL, "atx_regrid_csr_missing: %lld x %d items exceed one launch", (long long)n_tgt, C);
    const unsigned n_blocks = (unsigned)blocks;
    hipLaunchKernelGGL((regrid_cols_csr_missing_kernel<T, VEC>), dim3(n_blocks), dim3(kMissingBlock), 0, st, src, out, indptr, indices, data, n_items,
                       C, sp, op, n_blocks, heaviest ? 1 : 0, min_valid);
    ATX_LAUNCH_CHECK("regrid_cols_csr_missing");
    return ATX_OK;
}

template <typename T>
static int regrid_csr_missing_typed(const void* src_, void* out_, const int32_t* indptr, const int32_t* indices, const void* data_, int64_t n_tgt,
                                    int n_lev, int64_t sp, int64_t op, bool heaviest, double min_valid, hipStream_t st) {
    const T* src = static_cast<const T*>(src_);
    T* out = static_cast<T*>(out_);
    const T* data = static_cast<const T*>(data_);
    if (missing_vector_ok<T>(src_, out_, n_lev, sp, op))
        return launch_csr_missing<T, Vec16<T>::N>(src, out, indptr, indices, data, n_tgt, n_lev, sp, op, heaviest, static_cast<T>(min_valid), st);
    return launch_csr_missing<T, 1>(src, out, indptr, indices, data, n_tgt, n_lev, sp, op, heaviest, static_cast<T>(min_valid), st);
}

static int check_missing_args(const char* fn, int layout, int policy, double min_valid) {
    ATX_REQUIRE(policy == ATX_MISSING_ALL || policy == ATX_MISSING_HEAVIEST, ATX_EINVAL, "%s: unknown missing-value policy %d", fn, policy);
    ATX_REQUIRE(min_valid >= 0.0 && min_valid <= 1.0, ATX_EINVAL, "%s: min_valid = %g is outside [0, 1]", fn, min_valid);  // (NaN fails both)
    ATX_REQUIRE(layout == ATX_COLUMNS, ATX_ENOTIMPL, "%s: column stacks only (convert an ATX_FIELDS stack with atx_relayout)", fn);
    return ATX_OK;
}

}  // namespace atx

using namespace atx;

extern "C" int atx_missing_version(void) { return ATX_MISSING_VERSION; }

extern "C" const char* atx_missing_last_error(void) { return last_error().c_str(); }

extern "C" int atx_regrid_ell_missing(const void* src, void* out, const int32_t* idx, const void* w, int64_t n_src, int64_t n_tgt, int32_t k,
                                      int64_t n_lev, int64_t src_pitch, int64_t out_pitch, int dtype, int layout, int32_t flags, int policy,
                                      double min_valid, void* stream) {
    const char* fn = "atx_regrid_ell_missing";
    int st = check_stack_args(fn, src, out, n_src, n_tgt, n_lev, src_pitch, out_pitch, dtype, layout);
    if (st != ATX_OK) return st;
    ATX_REQUIRE(idx || n_tgt == 0, ATX_EINVAL, "%s: null idx", fn);
    ATX_REQUIRE(k >= 1 && k <= 64, ATX_EINVAL, "%s: k=%d outside [1, 64]", fn, k);
    ATX_REQUIRE(w, ATX_EINVAL, "%s: null w (an unweighted gather has nothing to renormalise: use atx_regrid_ell)", fn);
    ATX_REQUIRE((flags & ~ATX_ELL_PADDED) == 0, ATX_EINVAL, "%s: unknown flags 0x%x", fn, flags);
    st = check_missing_args(fn, layout, policy, min_valid);
    if (st != ATX_OK) return st;
    if (n_tgt == 0) return ATX_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (validation_on()) {
        st = validate_table(fn, "idx", idx, n_tgt * k, (flags & ATX_ELL_PADDED) ? -1 : 0, n_src, s);
        if (st != ATX_OK) return st;
    }
    const bool heaviest = policy == ATX_MISSING_HEAVIEST;
    if (dtype == ATX_F32) return regrid_ell_missing_typed<float>(src, out, idx, w, n_tgt, k, (int)n_lev, src_pitch, out_pitch, heaviest, min_valid, s);
    return regrid_ell_missing_typed<double>(src, out, idx, w, n_tgt, k, (int)n_lev, src_pitch, out_pitch, heaviest, min_valid, s);
}

extern "C" int atx_regrid_csr_missing(const void* src, void* out, const int32_t* indptr, const int32_t* indices, const void* data, int64_t n_src,
                                      int64_t n_tgt, int64_t nnz, int64_t n_lev, int64_t src_pitch, int64_t out_pitch, int dtype, int layout,
                                      int policy, double min_valid, void* stream) {
    const char* fn = "atx_regrid_csr_missing";
    int st = check_stack_args(fn, src, out, n_src, n_tgt, n_lev, src_pitch, out_pitch, dtype, layout);
    if (st != ATX_OK) return st;
    ATX_REQUIRE(indptr || n_tgt == 0, ATX_EINVAL, "%s: null indptr", fn);
    ATX_REQUIRE(nnz >= 0 && nnz <= INT32_MAX, ATX_ENOTIMPL, "%s: nnz=%lld outside int32", fn, (long long)nnz);
    ATX_REQUIRE(nnz == 0 || (indices && data), ATX_EINVAL, "%s: null indices/data", fn);
    st = check_missing_args(fn, layout, policy, min_valid);
    if (st != ATX_OK) return st;
    if (n_tgt == 0) return ATX_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (validation_on()) {
        st = validate_table(fn, "indices", indices, nnz, 0, n_src, s);
        if (st == ATX_OK) st = validate_table(fn, "indptr", indptr, n_tgt + 1, 0, nnz + 1, s);
        if (st != ATX_OK) return st;
    }
    const bool heaviest = policy == ATX_MISSING_HEAVIEST;
    if (dtype == ATX_F32)
        return regrid_csr_missing_typed<float>(src, out, indptr, indices, data, n_tgt, (int)n_lev, src_pitch, out_pitch, heaviest, min_valid, s);
    return regrid_csr_missing_typed<double>(src, out, indptr, indices, data, n_tgt, (int)n_lev, src_pitch, out_pitch, heaviest, min_valid, s);
}
