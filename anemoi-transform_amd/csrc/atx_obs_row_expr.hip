// filter_query and mask_values_custom: a POSTFIX expression program over float64 columns, one launch, and the
// ascending positions of the rows it keeps, a second one: atx_obs_row_expr and atx_obs_keep_positions, with their argument checks at the
// end of this file.  The instruction set is atx_expr_op (include/atx.h): pushes of a
// column or a constant, + - * /, negate, abs, round-to-float32, the six compares, membership in a slice of the constant table, and /
// or / not, DUP / SWAP for chained compares, and NAN_WHERE for Series.mask.
//
// The reference (R: filters/tabular/filter_query.py: obs_df.query(query); mask_values_custom.py: obs_df.eval(condition) and
// Series.mask) hands the text to pandas, whose python engine evaluates it node by node with numpy: one pass over the table and one
// temporary per node.  Here the whole expression is ONE pass, every intermediate in registers.
//
// Arithmetic: each of + - * / is one IEEE float64 operation; contraction is off for this file (a*b + c rounds twice, as numpy does).
// A float32 node of the expression is its float64 operation followed by ROUND_F32: for + - * / of float32 operands the double rounding
// is innocuous (53 >= 2*24 + 2), so the bits are numpy's float32 ones, subnormals included.  Compares are IEEE's: false against a NaN,
// except NE.  NEG, ABS and the select of NAN_WHERE work on bits: a NaN keeps its payload; the only value made is NAN_WHERE's canonical
// quiet NaN, which is what Series.mask writes.
//
// THE STACK IS IN REGISTERS, by a compare-select chain: the top of the stack is one register, the ATX_EXPR_MAX_STACK - 1 slots below it
// are seven separate doubles — a read or write at the (uniform) run-time depth d is a chain of `k == d ? ... : ...` over the 7 slots.  The depth depends on the program alone, so it lives in a scalar register and
// every such compare is a scalar one.  A private array with a run-time subscript would go to scratch memory (or, promoted, to 14 KB of
// LDS per workgroup); this stack does neither (tools/kernel_resources.py reports 0 bytes of scratch and 16 bytes of LDS, the four
// popcounts of a chunk; tests/test_host_api.py checks every kernel of the library for scratch).
//
// Launch shape: the per-row kernels' (atx_obs_rows.hpp): kBlock lanes, row_grid, grid-stride, one lane per row.  The program is uniform
// over the launch: every branch on it is scalar and every constant read is a scalar load.  The loop bound is uniform per workgroup, so
// every lane of a wave reaches the ballot; a lane at or past n loads nothing and contributes a 0 bit.  One workgroup iteration covers
// exactly one chunk of ATX_EXPR_CHUNK_ROWS = kBlock rows: lane 0 of each wave stores the wave's 64-bit word, and thread 0 the sum of the
// four popcounts as the chunk's count.  No atomics, no order between workgroups; stores are plain vector stores; no __restrict__, since
// out[r] may be any in[k].
#include "atx_obs_rows.hpp"

#pragma clang fp contract(off)

namespace atx {

static_assert(ATX_EXPR_CHUNK_ROWS == kBlock, "one workgroup iteration owns one chunk");
static_assert(kBlock % kWave == 0, "whole waves");
constexpr int kBelow = ATX_EXPR_MAX_STACK - 1;  // the slots under the top register
constexpr int kChunkWords = ATX_EXPR_CHUNK_ROWS / kWave;

// The program of one launch, by value in the kernel arguments (about 1.1 KB).  Everything indexed at run time is dwords or qwords, so a
// scalar load fetches it.
struct ExprProgram {
    const double* in[ATX_EXPR_MAX_INPUTS];
    double* out[ATX_EXPR_MAX_RESULTS];
    double consts[ATX_EXPR_MAX_CONSTS];
    int32_t code[ATX_EXPR_MAX_INSTR];
    int32_t arg0[ATX_EXPR_MAX_INSTR];
    int32_t arg1[ATX_EXPR_MAX_INSTR];
    int32_t n_instr;
    int32_t n_results;
    unsigned long long* keep_words;  // with its chunk_counts, or both null
    int64_t* chunk_counts;
};

// Seven separate locals, not an array or a struct: the compiler folds a select chain over the members of ONE private object back into
// a load at a run-time offset, and then moves the object into LDS (14 KB per workgroup) or scratch.
static_assert(kBelow == 7, "the kernel names its slots");
#define ATX_BELOW_GET(k) below_get(k, s0, s1, s2, s3, s4, s5, s6)
#define ATX_BELOW_SET(k, v) below_set(k, v, s0, s1, s2, s3, s4, s5, s6)

__device__ __forceinline__ double below_get(int k, double s0, double s1, double s2, double s3, double s4, double s5, double s6) {
    double v = s0;
    v = (k == 1) ? s1 : v;
    v = (k == 2) ? s2 : v;
    v = (k == 3) ? s3 : v;
    v = (k == 4) ? s4 : v;
    v = (k == 5) ? s5 : v;
    v = (k == 6) ? s6 : v;
    return v;
}

__device__ __forceinline__ void below_set(int k, double v, double& s0, double& s1, double& s2, double& s3, double& s4, double& s5, double& s6) {
    s0 = (k == 0) ? v : s0;
    s1 = (k == 1) ? v : s1;
    s2 = (k == 2) ? v : s2;
    s3 = (k == 3) ? v : s3;
    s4 = (k == 4) ? v : s4;
    s5 = (k == 5) ? v : s5;
    s6 = (k == 6) ? v : s6;
}

__device__ __forceinline__ double expr_flag(bool c) { return c ? 1.0 : 0.0; }

__device__ __forceinline__ double expr_binary(int op, double x, double y) {
    switch (op) {
        case ATX_EXPR_ADD: return x + y;
        case ATX_EXPR_SUB: return x - y;
        case ATX_EXPR_MUL: return x * y;
        case ATX_EXPR_DIV: return x / y;
        case ATX_EXPR_CMP_GT: return expr_flag(x > y);
        case ATX_EXPR_CMP_LT: return expr_flag(x < y);
        case ATX_EXPR_CMP_EQ: return expr_flag(x == y);
        case ATX_EXPR_CMP_NE: return expr_flag(x != y);
        case ATX_EXPR_CMP_GE: return expr_flag(x >= y);
        case ATX_EXPR_CMP_LE: return expr_flag(x <= y);
        case ATX_EXPR_AND: return expr_flag(x != 0.0 && y != 0.0);
        case ATX_EXPR_OR: return expr_flag(x != 0.0 || y != 0.0);
        default: return y != 0.0 ? __longlong_as_double(0x7ff8000000000000ll) : x;  // NAN_WHERE
    }
}

__device__ __forceinline__ bool expr_is_binary(int op) {
    return (op >= ATX_EXPR_ADD && op <= ATX_EXPR_DIV) || (op >= ATX_EXPR_CMP_GT && op <= ATX_EXPR_CMP_LE) || op == ATX_EXPR_AND ||
           op == ATX_EXPR_OR || op == ATX_EXPR_NAN_WHERE;
}

__global__ void __launch_bounds__(kBlock) obs_row_expr_kernel(const ExprProgram p, int64_t n) {
    __shared__ int wave_kept[kBlock / kWave];
    const bool keep = p.keep_words != nullptr;
    for (int64_t base = (int64_t)blockIdx.x * kBlock; base < n; base += (int64_t)gridDim.x * kBlock) {
        const int64_t i = base + threadIdx.x;
        const bool live = i < n;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0, s5 = 0.0, s6 = 0.0;
        double top = 0.0;
        int d = 0;  // the depth: top is slot d - 1, sk slot k < d - 1
        for (int t = 0; t < ATX_EXPR_MAX_INSTR; ++t) {
            if (t >= p.n_instr) break;
            const int op = p.code[t];
            const int a = p.arg0[t];
            if (op == ATX_EXPR_PUSH_COL || op == ATX_EXPR_PUSH_CONST || op == ATX_EXPR_DUP) {
                double v;
                if (op == ATX_EXPR_PUSH_COL) {
                    v = live ? p.in[a][i] : 0.0;
                } else if (op == ATX_EXPR_PUSH_CONST) {
                    v = p.consts[a];
                } else {
                    v = a == 0 ? top : ATX_BELOW_GET(d - 1 - a);
                }
                if (d > 0) ATX_BELOW_SET(d - 1, top);
                top = v;
                ++d;
            } else if (expr_is_binary(op)) {
                top = expr_binary(op, ATX_BELOW_GET(d - 2), top);
                --d;
            } else if (op == ATX_EXPR_SWAP) {
                const double x = ATX_BELOW_GET(d - 2);
                ATX_BELOW_SET(d - 2, top);
                top = x;
            } else if (op == ATX_EXPR_IN_SET) {
                bool hit = false;
                const int end = a + p.arg1[t];
                for (int j = a; j < end; ++j) hit = hit || (top == p.consts[j]);
                top = expr_flag(hit);
            } else if (op == ATX_EXPR_NEG) {
                top = __longlong_as_double(__double_as_longlong(top) ^ (long long)0x8000000000000000ull);
            } else if (op == ATX_EXPR_ABS) {
                top = __longlong_as_double(__double_as_longlong(top) & 0x7fffffffffffffffll);
            } else if (op == ATX_EXPR_ROUND_F32) {
                top = (double)(float)top;
            } else {  // NOT
                top = expr_flag(top == 0.0);
            }
        }
        // the host has checked: d == n_results (+ 1 with keep), so slot r < n_results - 1 + keep lies below the top
        for (int r = 0; r < ATX_EXPR_MAX_RESULTS; ++r) {
            if (r >= p.n_results) break;
            const double v = (r == d - 1) ? top : ATX_BELOW_GET(r);
            if (live) p.out[r][i] = v;
        }
        if (keep) {
            const unsigned long long word = __ballot(live && top != 0.0);
            const int wave = threadIdx.x / kWave;
            if (threadIdx.x % kWave == 0) {
                if (base + (int64_t)wave * kWave < n) p.keep_words[(base >> 6) + wave] = word;
                wave_kept[wave] = __popcll(word);
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                int kept = 0;
                for (int w = 0; w < kBlock / kWave; ++w) kept += wave_kept[w];
                p.chunk_counts[base / ATX_EXPR_CHUNK_ROWS] = kept;
            }
            __syncthreads();  // wave_kept is written again in the next iteration
        }
    }
}

// One lane per row.  The word of a row is one address per wave (rows 64 w .. 64 w + 63: kBlock and the chunk are multiples of 64).
__global__ void __launch_bounds__(kBlock) obs_keep_positions_kernel(const unsigned long long* words, const int64_t* chunk_offsets, int64_t n,
                                                                    int64_t* positions, int64_t n_positions) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const int64_t w = i >> 6;
        const int lane = (int)(i & 63);
        const unsigned long long word = words[w];
        if (!((word >> lane) & 1ull)) continue;
        const int64_t chunk = i / ATX_EXPR_CHUNK_ROWS;
        int64_t place = chunk_offsets[chunk] + __popcll(word & ((1ull << lane) - 1ull));
        for (int64_t v = chunk * kChunkWords; v < w; ++v) place += __popcll(words[v]);
        if (place >= 0 && place < n_positions) positions[place] = i;
    }
}

}  // namespace atx

using namespace atx;

// Everything is validated, the stack depth by simulation, before anything touches HIP.
extern "C" int atx_obs_row_expr(int32_t n_instr, const int32_t* code, const int32_t* arg0, const int32_t* arg1, int32_t n_inputs,
                                const double* const* in, int32_t n_consts, const double* consts, int32_t n_results, double* const* out, int keep,
                                uint64_t* keep_words, int64_t* chunk_counts, int64_t n, void* stream) {
    ATX_REQUIRE(n >= 0, ATX_EINVAL, "atx_obs_row_expr: %lld rows", (long long)n);
    ATX_REQUIRE(code && arg0 && arg1, ATX_EINVAL, "atx_obs_row_expr: null program array");
    ATX_REQUIRE(n_instr >= 1 && n_instr <= ATX_EXPR_MAX_INSTR, ATX_EINVAL, "atx_obs_row_expr: 1 .. %d instructions, got %d", ATX_EXPR_MAX_INSTR,
                (int)n_instr);
    ATX_REQUIRE(n_inputs >= 0 && n_inputs <= ATX_EXPR_MAX_INPUTS, ATX_EINVAL, "atx_obs_row_expr: 0 .. %d input columns, got %d", ATX_EXPR_MAX_INPUTS,
                (int)n_inputs);
    ATX_REQUIRE(n_consts >= 0 && n_consts <= ATX_EXPR_MAX_CONSTS, ATX_EINVAL, "atx_obs_row_expr: 0 .. %d constants, got %d", ATX_EXPR_MAX_CONSTS,
                (int)n_consts);
    ATX_REQUIRE(n_results >= 0 && n_results <= ATX_EXPR_MAX_RESULTS, ATX_EINVAL, "atx_obs_row_expr: 0 .. %d value results, got %d",
                ATX_EXPR_MAX_RESULTS, (int)n_results);
    ATX_REQUIRE(n_results > 0 || keep, ATX_EINVAL, "atx_obs_row_expr: neither a value result nor a keep condition is asked for");
    ATX_REQUIRE((in || n_inputs == 0) && (consts || n_consts == 0) && (out || n_results == 0), ATX_EINVAL, "atx_obs_row_expr: null table");
    ATX_REQUIRE(!keep || (keep_words && chunk_counts) || n == 0, ATX_EINVAL, "atx_obs_row_expr: a null keep_words or chunk_counts row");
    ExprProgram p = {};
    int depth = 0;
    for (int t = 0; t < n_instr; ++t) {
        const int op = code[t];
        ATX_REQUIRE(op >= ATX_EXPR_PUSH_COL && op <= ATX_EXPR_NAN_WHERE, ATX_EINVAL, "atx_obs_row_expr: instruction %d has the unknown code %d", t, op);
        int pops = 1, pushes = 1;  // the unary ones
        if (op == ATX_EXPR_PUSH_COL) {
            ATX_REQUIRE(arg0[t] >= 0 && arg0[t] < n_inputs, ATX_EINVAL, "atx_obs_row_expr: instruction %d reads column %d of %d", t, (int)arg0[t],
                        (int)n_inputs);
            pops = 0;
        } else if (op == ATX_EXPR_PUSH_CONST) {
            ATX_REQUIRE(arg0[t] >= 0 && arg0[t] < n_consts, ATX_EINVAL, "atx_obs_row_expr: instruction %d reads constant %d of %d", t, (int)arg0[t],
                        (int)n_consts);
            pops = 0;
        } else if (op == ATX_EXPR_DUP) {
            ATX_REQUIRE(arg0[t] >= 0 && arg0[t] < depth, ATX_EINVAL,
                        "atx_obs_row_expr: instruction %d copies the value %d below the top of a stack of %d: stack underflow", t, (int)arg0[t], depth);
            pops = 0;
        } else if (op == ATX_EXPR_IN_SET) {
            ATX_REQUIRE(arg0[t] >= 0 && arg1[t] >= 1 && (int64_t)arg0[t] + arg1[t] <= n_consts, ATX_EINVAL,
                        "atx_obs_row_expr: instruction %d: the IN_SET slice [%d, %d + %d) lies outside the table of %d constants", t, (int)arg0[t],
                        (int)arg0[t], (int)arg1[t], (int)n_consts);
        } else if (op == ATX_EXPR_SWAP) {
            pops = pushes = 2;
        } else if (op != ATX_EXPR_NEG && op != ATX_EXPR_ABS && op != ATX_EXPR_ROUND_F32 && op != ATX_EXPR_NOT) {
            pops = 2;  // + - * /, the compares, AND, OR, NAN_WHERE
        }
        ATX_REQUIRE(depth >= pops, ATX_EINVAL, "atx_obs_row_expr: instruction %d (code %d) takes %d values of a stack of %d: stack underflow", t, op, pops,
                    depth);
        depth += pushes - pops;
        ATX_REQUIRE(depth <= ATX_EXPR_MAX_STACK, ATX_EINVAL, "atx_obs_row_expr: instruction %d: stack overflow, the depth is at most %d", t,
                    ATX_EXPR_MAX_STACK);
        p.code[t] = op;
        p.arg0[t] = arg0[t];
        p.arg1[t] = op == ATX_EXPR_IN_SET ? arg1[t] : 0;
    }
    ATX_REQUIRE(depth == n_results + (keep ? 1 : 0), ATX_EINVAL, "atx_obs_row_expr: the program leaves %d values, %d value results%s are asked for", depth,
                (int)n_results, keep ? " and a keep condition" : "");
    for (int k = 0; k < n_inputs; ++k) {
        ATX_REQUIRE(in[k] || n == 0, ATX_EINVAL, "atx_obs_row_expr: null input column %d", k);
        p.in[k] = in[k];
    }
    for (int r = 0; r < n_results; ++r) {
        ATX_REQUIRE(out[r] || n == 0, ATX_EINVAL, "atx_obs_row_expr: output row %d is null", r);
        p.out[r] = out[r];
    }
    for (int k = 0; k < n_consts; ++k) p.consts[k] = consts[k];
    p.n_instr = n_instr;
    p.n_results = n_results;
    p.keep_words = keep ? reinterpret_cast<unsigned long long*>(keep_words) : nullptr;
    p.chunk_counts = keep ? chunk_counts : nullptr;
    if (n == 0) return ATX_OK;
    hipLaunchKernelGGL(obs_row_expr_kernel, dim3(row_grid(n)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), p, n);
    ATX_LAUNCH_CHECK("obs_row_expr");
    return ATX_OK;
}

extern "C" int atx_obs_keep_positions(const uint64_t* keep_words, const int64_t* chunk_offsets, int64_t n, int64_t* positions, int64_t n_positions,
                                      void* stream) {
    ATX_REQUIRE(n >= 0 && n_positions >= 0, ATX_EINVAL, "atx_obs_keep_positions: %lld rows, %lld positions", (long long)n, (long long)n_positions);
    if (n == 0 || n_positions == 0) return ATX_OK;
    ATX_REQUIRE(keep_words && chunk_offsets && positions, ATX_EINVAL, "atx_obs_keep_positions: null pointer");
    hipLaunchKernelGGL(obs_keep_positions_kernel, dim3(row_grid(n)), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const unsigned long long*>(keep_words), chunk_offsets, n, positions, n_positions);
    ATX_LAUNCH_CHECK("obs_keep_positions");
    return ATX_OK;
}
