// Library-level entry points of libatx: version, error strings, device probe.
#include "atx_common.hpp"
#include "atx_obs_rows.hpp"

#include <cstring>
#include <string>

namespace atx {

static thread_local std::string g_last_error;
// The launch form the calling thread's last atx_pointwise_stack took (atx_last_route): a literal, set by the dispatcher of
// atx_pointwise.hip.  Diagnostic only.
__thread const char* g_last_route = "none";

void set_error(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
}

int hip_status(hipError_t e, const char* what) {
    if (e == hipSuccess) return ATX_OK;
    set_error("%s: HIP error %d (%s)", what, (int)e, hipGetErrorString(e));
    return ATX_EHIP;
}

}  // namespace atx

extern "C" int atx_version(void) { return ATX_VERSION; }

extern "C" const char* atx_last_error(void) { return atx::g_last_error.c_str(); }

extern "C" const char* atx_last_route(void) { return atx::g_last_route; }

extern "C" const char* atx_strerror(int code) {
    switch (code) {
        case ATX_OK: return "ok";
        case ATX_EINVAL: return "invalid argument";
        case ATX_ESHAPE: return "shape mismatch";
        case ATX_ENOTIMPL: return "not implemented";
        case ATX_EHIP: return "HIP runtime error";
        case ATX_EALIGN: return "alignment requirement not met";
        case ATX_EWORKSPACE: return "workspace too small";
        case ATX_ECOMM: return "RCCL unavailable or collective failed";
        default: return "unknown error";
    }
}

extern "C" int atx_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        // no device / no driver is an answer, not a failure of the probe
        (void)hipGetLastError();
        if (e == hipErrorNoDevice) return 0;
        return atx::hip_status(e, "hipGetDeviceCount");
    }
    return n;
}

extern "C" int64_t atx_vector_program(const atx_level_op* prog, int32_t n_stage, int64_t n_lev, int dtype, atx_level_op* out, int64_t out_entries) {
    if (!prog || n_stage < 1 || n_stage > 8 || n_lev < 1 || (dtype != ATX_F32 && dtype != ATX_F64)) {
        atx::set_error("atx_vector_program: bad arguments (n_stage=%d, n_lev=%lld, dtype=%d)", n_stage, (long long)n_lev, dtype);
        return ATX_EINVAL;
    }
    const int64_t V = dtype == ATX_F32 ? 4 : 2;
    const int64_t C = (n_lev + V - 1) / V;
    const atx::LevelTables lay = atx::level_tables_layout(n_stage, n_lev, dtype);
    const int64_t n_entries = (lay.total_bytes + (int64_t)sizeof(atx_level_op) - 1) / (int64_t)sizeof(atx_level_op);
    if (!out) return n_entries;
    if (out_entries < n_entries) {  // never write past what the caller says it allocated (0.3 had no capacity argument)
        atx::set_error("atx_vector_program: out holds %lld entries, the table needs %lld (size it with the out == NULL query)",
                       (long long)out_entries, (long long)n_entries);
        return ATX_EWORKSPACE;
    }
    // the same rule as the kernels' own table build (build_vector_ops): equality of op, use_mask and of the parameters AS
    // THE KERNEL WILL SEE THEM, i.e. after rounding to the stack's arithmetic type
    auto same_param = [dtype](double a, double b) {
        if (dtype == ATX_F32) {
            const float fa = (float)a, fb = (float)b;
            return std::memcmp(&fa, &fb, sizeof(float)) == 0;
        }
        return std::memcmp(&a, &b, sizeof(double)) == 0;
    };
    for (int32_t s = 0; s < n_stage; ++s) {
        for (int64_t c = 0; c < C; ++c) {
            const atx_level_op* first = prog + (int64_t)s * n_lev + c * V;
            atx_level_op o = *first;
            bool mixed = false;
            int any_mask = first->use_mask;
            for (int64_t e = 1; e < V && c * V + e < n_lev; ++e) {
                const atx_level_op& q = first[e];
                mixed = mixed || q.op != o.op || q.use_mask != o.use_mask || !same_param(q.p0, o.p0) || !same_param(q.p1, o.p1);
                any_mask |= q.use_mask;
            }
            if (mixed) {  // the kernel goes level by level through `prog`; it only needs to know whether any level wants the mask
                o.op = ATX_OP_MIXED;
                o.use_mask = any_mask;
            }
            out[(int64_t)s * C + c] = o;
        }
    }
    // second part: every level's operator in the stack's type (atx_common.hpp: level_tables_layout)
    unsigned char* base = reinterpret_cast<unsigned char*>(out);
    std::memset(base + (int64_t)n_stage * C * (int64_t)sizeof(atx_level_op), 0,
                (size_t)(n_entries * (int64_t)sizeof(atx_level_op) - (int64_t)n_stage * C * (int64_t)sizeof(atx_level_op)));
    const int64_t B = dtype == ATX_F32 ? 4 : 8;
    unsigned char* p0 = base + lay.levels_offset;
    unsigned char* p1 = p0 + (int64_t)n_stage * lay.Lp * B;
    unsigned char* code = p1 + (int64_t)n_stage * lay.Lp * B;
    for (int32_t s = 0; s < n_stage; ++s) {
        for (int64_t l = 0; l < lay.Lp; ++l) {
            const atx_level_op& o = prog[(int64_t)s * n_lev + (l < n_lev ? l : n_lev - 1)];
            const int64_t i = (int64_t)s * lay.Lp + l;
            if (dtype == ATX_F32) {
                const float a = (float)o.p0, b = (float)o.p1;
                std::memcpy(p0 + i * B, &a, sizeof a);
                std::memcpy(p1 + i * B, &b, sizeof b);
            } else {
                std::memcpy(p0 + i * B, &o.p0, sizeof(double));
                std::memcpy(p1 + i * B, &o.p1, sizeof(double));
            }
            code[i] = (unsigned char)((o.op & 0x7f) | (o.use_mask ? 0x80 : 0));
        }
    }
    return n_entries;
}

namespace atx {
struct alignas(16) Bytes16 {
    uint32_t w[4];
};
__global__ void __launch_bounds__(kBlock) stream_copy_kernel(const Bytes16* __restrict__ src, Bytes16* __restrict__ dst, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) dst[i] = src[i];
}
}  // namespace atx

extern "C" int atx_stream_copy(const void* src, void* dst, int64_t n_bytes, void* stream) {
    using namespace atx;
    ATX_REQUIRE((src && dst) || n_bytes == 0, ATX_EINVAL, "atx_stream_copy: null pointer");
    ATX_REQUIRE(n_bytes >= 0 && n_bytes % 16 == 0, ATX_EINVAL, "atx_stream_copy: n_bytes=%lld is not a multiple of 16", (long long)n_bytes);
    ATX_REQUIRE(aligned16(src) && aligned16(dst), ATX_EALIGN, "atx_stream_copy: pointers must be 16-byte aligned");
    const int64_t n = n_bytes / 16;
    if (n == 0) return ATX_OK;
    const int64_t blocks = (n + kBlock - 1) / kBlock;
    ATX_REQUIRE(blocks <= 0x7fffffffll, ATX_ENOTIMPL, "atx_stream_copy: %lld bytes exceed one launch", (long long)n_bytes);
    hipLaunchKernelGGL(stream_copy_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                       static_cast<const Bytes16*>(src), static_cast<Bytes16*>(dst), n);
    ATX_LAUNCH_CHECK("stream_copy");
    return ATX_OK;
}

// ---- row expressions: the third family of atx_obs_column_ops' codes.  atx_obs_column_ops.hip reads the slots into the flat program
// ---- that is validated here; the kernels are in atx_obs_row_expr.hip --------------------------------------------------------------------
namespace atx {

int obs_row_expr_call(int32_t n_instr, const int32_t* code, const int32_t* arg0, const int32_t* arg1, int32_t n_inputs,
                      const double* const* in, int32_t n_consts, const double* consts, int32_t n_results, double* const* out, bool keep,
                      uint64_t* keep_words, int64_t* chunk_counts, int64_t n, void* stream) {
    ATX_REQUIRE(n >= 0, ATX_EINVAL, "atx_obs_column_ops, row expression: %lld rows", (long long)n);
    ATX_REQUIRE(code && arg0 && arg1, ATX_EINVAL, "atx_obs_column_ops, row expression: null program array");
    ATX_REQUIRE(n_instr >= 1 && n_instr <= ATX_EXPR_MAX_INSTR, ATX_EINVAL, "atx_obs_column_ops, row expression: 1 .. %d instructions, got %d", ATX_EXPR_MAX_INSTR,
                (int)n_instr);
    ATX_REQUIRE(n_inputs >= 0 && n_inputs <= ATX_EXPR_MAX_INPUTS, ATX_EINVAL, "atx_obs_column_ops, row expression: 0 .. %d input columns, got %d",
                ATX_EXPR_MAX_INPUTS, (int)n_inputs);
    ATX_REQUIRE(n_consts >= 0 && n_consts <= ATX_EXPR_MAX_CONSTS, ATX_EINVAL, "atx_obs_column_ops, row expression: 0 .. %d constants, got %d", ATX_EXPR_MAX_CONSTS,
                (int)n_consts);
    ATX_REQUIRE(n_results >= 0 && n_results <= ATX_EXPR_MAX_RESULTS, ATX_EINVAL, "atx_obs_column_ops, row expression: 0 .. %d value results, got %d",
                ATX_EXPR_MAX_RESULTS, (int)n_results);
    ATX_REQUIRE(n_results > 0 || keep, ATX_EINVAL, "atx_obs_column_ops, row expression: neither a value result nor keep_words is asked for");
    ATX_REQUIRE((in || n_inputs == 0) && (consts || n_consts == 0) && (out || n_results == 0), ATX_EINVAL, "atx_obs_column_ops, row expression: null table");
    ATX_REQUIRE(!keep || (keep_words && chunk_counts) || n == 0, ATX_EINVAL, "atx_obs_column_ops, row expression: a null keep_words or chunk_counts row");
    ExprProgram p = {};
    int depth = 0;
    for (int t = 0; t < n_instr; ++t) {
        const int op = code[t];
        ATX_REQUIRE(op >= ATX_EXPR_PUSH_COL && op <= ATX_EXPR_NAN_WHERE, ATX_EINVAL, "atx_obs_column_ops, row expression: instruction %d has the unknown code %d", t, op);
        int pops = 1, pushes = 1;  // the unary ones
        if (op == ATX_EXPR_PUSH_COL) {
            ATX_REQUIRE(arg0[t] >= 0 && arg0[t] < n_inputs, ATX_EINVAL, "atx_obs_column_ops, row expression: instruction %d reads column %d of %d", t, (int)arg0[t],
                        (int)n_inputs);
            pops = 0;
        } else if (op == ATX_EXPR_PUSH_CONST) {
            ATX_REQUIRE(arg0[t] >= 0 && arg0[t] < n_consts, ATX_EINVAL, "atx_obs_column_ops, row expression: instruction %d reads constant %d of %d", t,
                        (int)arg0[t], (int)n_consts);
            pops = 0;
        } else if (op == ATX_EXPR_DUP) {
            ATX_REQUIRE(arg0[t] >= 0 && arg0[t] < depth, ATX_EINVAL, "atx_obs_column_ops, row expression: instruction %d copies the value %d below the top of a stack of %d: stack underflow",
                        t, (int)arg0[t], depth);
            pops = 0;
        } else if (op == ATX_EXPR_IN_SET) {
            ATX_REQUIRE(arg0[t] >= 0 && arg1[t] >= 1 && (int64_t)arg0[t] + arg1[t] <= n_consts, ATX_EINVAL,
                        "atx_obs_column_ops, row expression: instruction %d: the IN_SET slice [%d, %d + %d) lies outside the table of %d constants", t, (int)arg0[t],
                        (int)arg0[t], (int)arg1[t], (int)n_consts);
        } else if (op == ATX_EXPR_SWAP) {
            pops = pushes = 2;
        } else if (op != ATX_EXPR_NEG && op != ATX_EXPR_ABS && op != ATX_EXPR_ROUND_F32 && op != ATX_EXPR_NOT) {
            pops = 2;  // + - * /, the compares, AND, OR, NAN_WHERE
        }
        ATX_REQUIRE(depth >= pops, ATX_EINVAL, "atx_obs_column_ops, row expression: instruction %d (code %d) takes %d values of a stack of %d: stack underflow", t, op,
                    pops, depth);
        depth += pushes - pops;
        ATX_REQUIRE(depth <= ATX_EXPR_MAX_STACK, ATX_EINVAL, "atx_obs_column_ops, row expression: instruction %d: stack overflow, the depth is at most %d", t,
                    ATX_EXPR_MAX_STACK);
        p.code[t] = op;
        p.arg0[t] = arg0[t];
        p.arg1[t] = op == ATX_EXPR_IN_SET ? arg1[t] : 0;
    }
    ATX_REQUIRE(depth == n_results + (keep ? 1 : 0), ATX_EINVAL,
                "atx_obs_column_ops, row expression: the program leaves %d values, %d value results%s are asked for", depth, (int)n_results,
                keep ? " and a keep condition" : "");
    for (int k = 0; k < n_inputs; ++k) {
        ATX_REQUIRE(in[k] || n == 0, ATX_EINVAL, "atx_obs_column_ops, row expression: input column %d is null", k);
        p.in[k] = in[k];
    }
    for (int r = 0; r < n_results; ++r) {
        ATX_REQUIRE(out[r] || n == 0, ATX_EINVAL, "atx_obs_column_ops, row expression: output row %d is null", r);
        p.out[r] = out[r];
    }
    for (int k = 0; k < n_consts; ++k) p.consts[k] = consts[k];
    p.n_instr = n_instr;
    p.n_results = n_results;
    p.keep_words = keep ? reinterpret_cast<unsigned long long*>(keep_words) : nullptr;
    p.chunk_counts = keep ? chunk_counts : nullptr;
    if (n == 0) return ATX_OK;
    return launch_obs_row_expr(p, n, static_cast<hipStream_t>(stream));
}

int obs_keep_positions_call(const uint64_t* words, const int64_t* chunk_offsets, int64_t n, int64_t* positions, int64_t n_positions,
                            void* stream) {
    ATX_REQUIRE(n >= 0 && n_positions >= 0, ATX_EINVAL, "atx_obs_column_ops, keep positions: %lld rows, %lld positions", (long long)n, (long long)n_positions);
    if (n == 0 || n_positions == 0) return ATX_OK;
    ATX_REQUIRE(words && chunk_offsets && positions, ATX_EINVAL, "atx_obs_column_ops, keep positions: null pointer");
    return launch_obs_keep_positions(reinterpret_cast<const unsigned long long*>(words), chunk_offsets, n, positions, n_positions,
                                     static_cast<hipStream_t>(stream));
}

}  // namespace atx
