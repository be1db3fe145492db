// Shared by the three translation units of the regrid entry points (round 4: atx_regrid.hip took 70 s to compile — the whole build's
// critical path — so its kernels are instantiated per element type in atx_regrid_f32.hip / atx_regrid_f64.hip, which compile in
// parallel, and atx_regrid.hip keeps the C ABI): the batch and epilogue arguments, the two typed entry points, and the helpers the
// columns and fields pieces of the gather (atx_regrid_columns.inc, atx_regrid_fields.inc) have in common.
#ifndef ATX_REGRID_DECL_HPP
#define ATX_REGRID_DECL_HPP

#include "atx_common.hpp"

namespace atx {

constexpr int kMaxBatch = 16;
struct EllBatch {
    const void* src[kMaxBatch];
    void* out[kMaxBatch];
    int n;
};

// The fused per-level program as the launchers see it: `prog` (device, per level) is always there when n_stage > 0; the two
// optional companions let the direct kernel take the epilogue — `vec_prog` (device: atx_vector_program of the stack's dtype)
// and `host_prog` (HOST copy of `prog`: the only way the library can SEE the program without a device round trip).
struct Epilogue {
    const atx_level_op* prog = nullptr;
    const atx_level_op* vec_prog = nullptr;
    const atx_level_op* host_prog = nullptr;
    int n_stage = 0;
    const uint8_t* mask = nullptr;
    const int32_t* tgt_rows = nullptr;  // ordered traversal (atx_regrid_ell_ordered): table row t is output row tgt_rows[t]
};

extern thread_local int g_tile_override;  // atx_set_tuning; defined in atx_regrid.hip

// The launch form of the calling thread's last gather (atx_last_gather_route, a diagnostic): every launcher stores literals and plain
// integers here immediately before its launch — a few stores, no formatting; atx_regrid.hip builds the string when it is read.  It
// never decides anything.
struct GatherRoute {
    const char* table;     // "cols_ell", "cols_csr", "fields_ell", "fields_csr"; nullptr: nothing launched
    const char* kernel;    // "direct" / "tiled" (column stacks), "lanes" (fields_ell), "head4" / "head8" / "long" (fields_csr)
    const char* epilogue;  // "none", "uniform", "runs", "table" (direct), "lds" (tiled, column CSR), "global" (field-major)
    const char* width;     // "vec" / "scalar" (column stacks), "lane" (field-major: one target per lane)
    int k;                 // compile-time k as instantiated, 0: the runtime loop (and CSR rows)
    bool padded, weighted, stripe, ordered;
    bool split;            // the program did not fit beside the tile: plain gather, then atx_pointwise_stack (set by atx_regrid.hip)
};
extern __thread GatherRoute g_gather_route;  // defined in atx_regrid.hip

template <typename T>
int regrid_ell_typed(const EllBatch& batch, const int32_t* idx, const void* w_, int64_t n_tgt, int k,
                            int n_lev, int64_t sp, int64_t op, int layout, bool pad, const Epilogue& e, hipStream_t st);
template <typename T>
int regrid_csr_typed(const void* src_, void* out_, const int32_t* indptr, const int32_t* indices,
                            const void* data_, int64_t n_tgt, int64_t nnz, int n_lev, int64_t sp, int64_t op,
                            int layout, const atx_level_op* prog, int n_stage, const uint8_t* m, const int32_t* rows, hipStream_t st);

// A compile-time int handed to a generic lambda (the epilogue kind of the direct kernel's launch, the k of the ladders).
template <int N>
using IntTag = std::integral_constant<int, N>;

// ---- helpers of the kernel pieces ------------------------------------------------------------------------------------------------
template <typename T, int N>
struct NativeVec {
    typedef T type __attribute__((ext_vector_type(N)));
};
template <typename T>
struct NativeVec<T, 1> {
    typedef T type;
};

// Output vectors of a column stack: written once and never re-read by the launch, so non-temporal (+3 % over plain stores on the
// headline, profiles/r01_ab_variants.log, nt_store).  The SOURCE vectors are plain loads: non-temporal ones gained nothing at k = 1 and
// lost 3-6 % at k = 4 (same log, nt_src).
template <typename T, int N>
__device__ __forceinline__ void store_out(Pack<T, N>* p, const Pack<T, N>& v) {
    using NV = typename NativeVec<T, N>::type;
    __builtin_nontemporal_store(*reinterpret_cast<const NV*>(&v), reinterpret_cast<NV*>(p));
}
// (Write-through stores there — `sc1`, `sc0 sc1` — lost 2.4-5.3 % on k4f64 (3.7 %), k4f32, k1f64 and the slowest 1/8 shard, direct and tiled alike;
// `sc1 nt` measured +0.4-0.9 %, inside three times the parent's own round-to-round spread, so not adopted: profiles/store_policy_ab.json.
// The four policies as one -D knob: tools/experiments/gather_store_policy.patch.)
//
// One output element of the field-major fixed-k kernel (lane = target: a wave writes 64 consecutive elements of one field): written
// through and dropped from the XCD's L2 (`sc1 nt`), so that the source fills of the same launch do not find it there as a dirty
// line to evict.  +3.4-3.9 % on k4f64, +3.2 % k1f64, +6.1 % k1f32, k4f32 +1.6 % (inside its spread) over the plain store it replaces;
// `nt` alone +1.1-1.3 %, `sc1` +2.3 % (same file).  The compiler has no store with these bits, so it is assembly — one vector store,
// address and data in VGPRs; the compiler neither counts it nor pads it, and a store of 8 bytes or fewer needs no wait state before
// its data register is written again (the kernel stores inside its level loop).  The statement orders memory, so the loads of the next
// level no longer move above it: k = 4 f64 went from 64 to 34 VGPRs, f32 from 56 to 26 — measured as part of the same figures.
template <typename T>
__device__ __forceinline__ void store_field(T* p, T v) {
    static_assert(sizeof(T) == 8 || sizeof(T) == 4, "store_field: f64 / f32 elements");
    if constexpr (sizeof(T) == 8)
        asm volatile("global_store_dwordx2 %0, %1, off sc1 nt" : : "v"(p), "v"(v) : "memory");
    else
        asm volatile("global_store_dword %0, %1, off sc1 nt" : : "v"(p), "v"(v) : "memory");
}
// One source vector of the fixed-k kernels, a plain load.  Kept as a function: written in place, the same load costs three
// instantiations one or two registers (the copy out of the function is what the compiler sees differently).
template <typename T, int N>
__device__ __forceinline__ Pack<T, N> load_src(const T* p) {
    return *reinterpret_cast<const Pack<T, N>*>(p);
}
// Index / weight words of the TILED kernel, each read once by one workgroup: non-temporal, +2 % (nt_both in the same log).  The direct
// kernel reads a target's words from several lanes and waves and uses plain loads.
template <typename T>
__device__ __forceinline__ T load_once(const T* p) {
    return __builtin_nontemporal_load(p);
}

static int pick_tile(int64_t n_tgt, int C, bool epilogue) {
    // Small tiles win: ~560 (target, vector) items per 256-lane workgroup, i.e. 16 targets of
    // 137 f32 levels, rounded up to a multiple of 4 targets (measured on O1280 -> 0.25 deg:
    // tiles of 12 / 16 beat 10, 14, 18-32; 64/128/512-lane workgroups reach the same plateau at
    // the same items-per-lane ratio — profiles/r01_ab_variants.log, r01_ab_block_sizes.log).  More, shorter
    // workgroups keep more of them in different phases (index staging / gather / store).
    // With an epilogue every workgroup first builds its operator table (a second global-load latency before the
    // barrier): tiles 2.5x larger amortise it — 137 levels f32: 0.491 ms at 16 targets, 0.469 at 32-48; f64: 0.985 ms at 8,
    // 0.878 at 24 (profiles/r01_ab_epilogue.log).
    const int items = epilogue ? 1400 : 560;
    int tile = (items / C + 2) / 4 * 4;  // nearest multiple of 4 targets: 16 (40 with epilogue) for 137 f32 levels, 8 (20) for f64
    if (tile < 8) tile = 8;
    if (tile > 256) tile = 256;
    if ((int64_t)tile > n_tgt) tile = (int)n_tgt;
    return tile;
}

static int pick_lev_chunk(int n_lev) {
    // enough level chunks for >= ~4 workgroups per CU even on small grids, chunks >= 8 levels
    int chunks = (n_lev + 31) / 32;
    return (n_lev + chunks - 1) / chunks;
}

template <typename T>
static bool cols_vector_ok(const void* src, const void* out, int64_t sp, int64_t op) {
    constexpr int VEC = Vec16<T>::N;
    return aligned16(src) && aligned16(out) && (sp % VEC == 0) && (op % VEC == 0);
}

}  // namespace atx

#endif  // ATX_REGRID_DECL_HPP
