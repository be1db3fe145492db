// Per-point transforms over a stack of levels: the per-level program evaluator.
//
// Replaces the per-field Python map of the reference
//   R: filter.py:188-196        SingleFieldFilter._map_transform / forward
//   R: filters/fields/rescale.py:25,28   x*scale+offset, (x-offset)/scale
//   R: filters/fields/orog_to_z.py:59,77 x*g, x/g
//   R: filters/fields/clipper.py:69, impute_nans.py:53-54, lnsp_to_sp.py:47,65
//   R: filters/fields/apply_mask.py:183-185, glacier_mask.py:33  values[mask] = nan
// by ONE streaming pass over the stack: level l gets prog[s][l] for each stage s.
// HBM-bound: 16-byte loads/stores, grid-strided over up to kStreamGrid short workgroups; levels whose program is all-COPY are not touched when the
// operation is in place.  Nine kernels, each the fastest on some program shape; pointwise_columns lists them in the order they are tried.
#include "atx_common.hpp"
#include <algorithm>
#include <optional>
#include <type_traits>

namespace atx {

// Independent 16-byte loads a lane of the chunked kernels has in flight.  2: -13 %, 8: +-1 % (f32, 137 levels).
constexpr int kPwUnroll = 4;

template <typename T, int N>
__device__ __forceinline__ Pack<T, N> pw_load(const T* p) {
    return *reinterpret_cast<const Pack<T, N>*>(p);
}
template <typename T, int N>
__device__ __forceinline__ void pw_store(T* p, const Pack<T, N>& v) {
    *reinterpret_cast<Pack<T, N>*>(p) = v;
}

// (row, vector column) of vector slot vi in rows of `cols` slots.  The branch is uniform over the launch: a 32-bit division when
// every slot index fits.
__device__ __forceinline__ void split_row_col(int64_t vi, int64_t n_vec, int cols, int64_t& row, int& c) {
    if (n_vec <= 0xffffffffll) {
        const unsigned r = (unsigned)vi / (unsigned)cols;
        row = r;
        c = (int)((unsigned)vi - r * (unsigned)cols);
    } else {
        row = vi / cols;
        c = (int)(vi - row * cols);
    }
}

// ATX_COLUMNS.  A workgroup sweeps CONTIGUOUS chunks of rows (points).  Its lanes are laid over
// (row-in-pass, vector column): lane = r*Cg + c with Cg = min(C, 256) columns per pass and
// 256/Cg rows per pass, so consecutive lanes touch consecutive 16 B, a lane keeps its column(s) — its
// operators are loop invariant — and the kPwUnroll loads a lane has in flight are adjacent passes of
// the same chunk (NOT megabytes apart: a fixed large power-of-two distance between a lane's
// concurrent streams aliases onto the same HBM channels and cost 25 % here).  HBM-bound; what the
// kernel needs is memory-level parallelism: 4 independent 16-byte loads per lane.
template <typename T, int VEC>
__global__ void __launch_bounds__(kBlock)
pointwise_cols_kernel(const T* __restrict__ x, T* __restrict__ y, int64_t n_pts, int n_lev, int C,
                      int64_t x_pitch, int64_t y_pitch, const atx_level_op* __restrict__ prog, int n_stage,
                      const uint8_t* __restrict__ point_mask, int in_place) {
    using V = Pack<T, VEC>;
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x;
    const LevelTablesLds<T> tab = build_level_tables<T, VEC>(prog, smem, n_stage, n_lev, C, tid, kBlock);
    __syncthreads();

    const int Cg = C < kBlock ? C : kBlock;
    const int rows_per_pass = kBlock / Cg;
    const int r = tid / Cg;
    const int cl = tid - r * Cg;
    if (r >= rows_per_pass) return;  // lanes beyond the last whole row of a pass idle (after the barrier)
    const int64_t chunk = (int64_t)rows_per_pass * kPwUnroll;

    for (int c = cl; c < C; c += Cg) {
        const bool act = level_tables_active<T, VEC>(tab, n_stage, c);
        if (!act && in_place) continue;  // untouched levels of an in-place call: nothing to move
        for (int64_t row0 = (int64_t)blockIdx.x * chunk; row0 < n_pts; row0 += (int64_t)gridDim.x * chunk) {
            V v[kPwUnroll];
            int64_t pp[kPwUnroll];
            bool ok[kPwUnroll];
#pragma unroll
            for (int u = 0; u < kPwUnroll; ++u) {
                pp[u] = row0 + (int64_t)u * rows_per_pass + r;
                ok[u] = pp[u] < n_pts;
                if (!ok[u]) pp[u] = row0;
                v[u] = pw_load<T, VEC>(x + pp[u] * x_pitch + (int64_t)c * VEC);
            }
#pragma unroll
            for (int u = 0; u < kPwUnroll; ++u) {
                if (!ok[u]) continue;
                if (act) {
                    const bool masked = point_mask ? (point_mask[pp[u]] != 0) : false;
                    apply_level_tables<T, VEC>(tab, n_stage, c, v[u], masked);
                }
                pw_store<T, VEC>(y + pp[u] * y_pitch + (int64_t)c * VEC, v[u]);
            }
        }
    }
}

// ATX_COLUMNS with tight, equal pitches (pitch == C*VEC: what Stack.empty allocates): the stack is ONE contiguous run of
// n_pts*C vectors.  A workgroup sweeps 16 KB chunks of it (kBlock * kPwUnroll vectors = 128 whole cache lines when the
// base is line aligned), so no line is shared between workgroups — the row-chunk kernel above fetched 4.4 % and wrote
// 1.8 % more than the stack holds (boundary lines of its chunks, PMC counters in profiles/traffic.json) and idles
// kBlock % C lanes.  A lane's column changes from pass to pass; its operators come from the LDS table either way.
template <typename T, int VEC, bool TRANS>
__global__ void __launch_bounds__(kBlock)
pointwise_cols_flat_kernel(const T* __restrict__ x, T* __restrict__ y, int64_t n_pts, int n_lev, int C,
                           const atx_level_op* __restrict__ prog, int n_stage,
                           const uint8_t* __restrict__ point_mask, int in_place) {
    using V = Pack<T, VEC>;
    extern __shared__ __align__(16) unsigned char smem[];
    LevelOp<T>* vec_ops = reinterpret_cast<LevelOp<T>*>(smem);  // [n_stage][C]
    uint8_t* active = reinterpret_cast<uint8_t*>(vec_ops + (size_t)n_stage * C);  // [C]: column has a non-COPY stage
    const int tid = threadIdx.x;
    build_vector_ops<T, VEC>(prog, vec_ops, n_stage, n_lev, C, tid, kBlock);
    __syncthreads();
    for (int c = tid; c < C; c += kBlock) {
        bool act = false;
        for (int s = 0; s < n_stage; ++s) {
            const LevelOp<T> o = vec_ops[s * C + c];
            act = act || o.op != ATX_OP_COPY || o.use_mask != 0;
        }
        active[c] = act ? 1 : 0;
    }
    __syncthreads();

    const int64_t n_vec = n_pts * C;
    constexpr int64_t kChunk = (int64_t)kBlock * kPwUnroll;
    // A workgroup takes every gridDim.x-th chunk: under the 65536-workgroup cap the stride is exactly 1 GiB, but a contiguous run of
    // chunks per workgroup measured 10 % SLOWER (2.68 against 2.43 ms, 137 float64 levels of O1280; profiles/r03_pointwise_ab_README.md).
    for (int64_t base = (int64_t)blockIdx.x * kChunk; base < n_vec; base += (int64_t)gridDim.x * kChunk) {
        const int64_t row_b = base / C;  // uniform: scalar unit
        const int col_b = (int)(base - row_b * C);
        V v[kPwUnroll];
        int64_t row[kPwUnroll];
        int col[kPwUnroll];
        bool ok[kPwUnroll], act[kPwUnroll];
#pragma unroll
        for (int u = 0; u < kPwUnroll; ++u) {
            const int off = col_b + u * kBlock + tid;  // < C + kChunk: 32-bit arithmetic
            const int dr = off / C;
            col[u] = off - dr * C;
            row[u] = row_b + dr;
            const int64_t vi = base + u * kBlock + tid;
            ok[u] = vi < n_vec;
            act[u] = active[col[u]] != 0;
            if (in_place && !act[u]) ok[u] = false;  // untouched levels of an in-place call: nothing to move
            if (ok[u]) v[u] = pw_load<T, VEC>(x + vi * VEC);
        }
#pragma unroll
        for (int u = 0; u < kPwUnroll; ++u) {
            if (!ok[u]) continue;
            if (act[u]) {
                const bool masked = point_mask ? (point_mask[row[u]] != 0) : false;
                apply_program_vec<T, VEC, TRANS>(vec_ops, prog, n_stage, n_lev, C, col[u], v[u], masked);
            }
            pw_store<T, VEC>(y + (base + u * kBlock + tid) * VEC, v[u]);
        }
    }
}

// The chunked sweep above with the operators of EVERY LEVEL staged in LDS, parameters and operator codes in separate arrays
// (p0[stage][level], p1[stage][level] in the stack's type, one byte op | mask << 7 per level): a lane fetches the parameters of the
// VEC levels of its vector with two conflict-free 16-byte LDS reads and their codes with one 2- / 4-byte read per stage.  A program
// with a different scale per level — what the packed surface stacks and fused pipelines produce — made every vector "mixed" on the
// kernel above: VEC x 24 bytes of operators per stage and vector out of L1 for 32 bytes of HBM traffic (137 levels of O1280, a scale
// per level: f32 1.88 ms = 0.48, f64 2.69 ms = 0.67); array-of-struct operators in LDS had been tried and lost to bank conflicts.
// NT (non-temporal loads and stores of the stack): float32 only, and not for an in-place call that skips untouched vectors —
// measured per case in profiles/r03_per_level_programs.log (f32 in place 0.68 -> 0.74, out of place 0.75 -> 0.76; f64 0.76 -> 0.73,
// in place with skipped vectors 0.71 -> 0.48).
template <typename T, int VEC, bool TRANS, bool NT>
__global__ void __launch_bounds__(kBlock)
pointwise_cols_levels_kernel(const T* __restrict__ x, T* __restrict__ y, int64_t n_pts, int n_lev, int C, int Cp,
                             const atx_level_op* __restrict__ prog, int n_stage,
                             const uint8_t* __restrict__ point_mask, int in_place) {
    // Cp >= C: vector slots per row (pitch / VEC) — slots beyond the C that hold levels are padding: neither read nor written
    using V = Pack<T, VEC>;
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x;
    const LevelTablesLds<T> tab = build_level_tables<T, VEC>(prog, smem, n_stage, n_lev, C, tid, kBlock);
    uint8_t* active = smem + level_tables_lds_bytes<T>(n_stage, C, VEC);  // [C]: the vector has a level that is not a plain COPY
    __syncthreads();
    for (int c = tid; c < C; c += kBlock) active[c] = level_tables_active<T, VEC>(tab, n_stage, c) ? 1 : 0;
    __syncthreads();

    const int64_t n_vec = n_pts * Cp;
    constexpr int64_t kChunk = (int64_t)kBlock * kPwUnroll;
    for (int64_t base = (int64_t)blockIdx.x * kChunk; base < n_vec; base += (int64_t)gridDim.x * kChunk) {
        const int64_t row_b = base / Cp;  // uniform: scalar unit
        const int col_b = (int)(base - row_b * Cp);
        V v[kPwUnroll];
        int64_t row[kPwUnroll];
        int col[kPwUnroll];
        bool ok[kPwUnroll], act[kPwUnroll];
#pragma unroll
        for (int u = 0; u < kPwUnroll; ++u) {
            const int off = col_b + u * kBlock + tid;  // < Cp + kChunk: 32-bit arithmetic
            const int dr = off / Cp;
            col[u] = off - dr * Cp;
            row[u] = row_b + dr;
            const int64_t vi = base + u * kBlock + tid;
            ok[u] = vi < n_vec && col[u] < C;
            if (col[u] >= C) col[u] = 0;
            act[u] = active[col[u]] != 0;
            if (in_place && !act[u]) ok[u] = false;  // untouched levels of an in-place call: nothing to move
            if (ok[u]) v[u] = NT ? pw_load_nt<T, VEC>(x + vi * VEC) : pw_load<T, VEC>(x + vi * VEC);
        }
#pragma unroll
        for (int u = 0; u < kPwUnroll; ++u) {
            if (!ok[u]) continue;
            if (act[u]) {
                const bool masked = point_mask ? (point_mask[row[u]] != 0) : false;
                apply_level_tables<T, VEC, TRANS>(tab, n_stage, col[u], v[u], masked);
            }
            if (NT) pw_store_nt<T, VEC>(y + (base + u * kBlock + tid) * VEC, v[u]);
            else pw_store<T, VEC>(y + (base + u * kBlock + tid) * VEC, v[u]);
        }
    }
}

// The same stacks with the per-vector operator table GIVEN (vec_prog, built once on the host by atx_vector_program): no
// shared memory, no barrier, no loop — one 16-byte vector per lane and one workgroup per 4 KB, the launch shape that
// streams fastest on MI355X (a plain y = a*x + b over 3.7 GB: 6.17 TB/s in this shape, 5.8 TB/s with 2-8 vectors per
// lane and / or a grid-stride loop — tools/experiments/stream_shapes.hip).  A lane fetches the operators of its column
// for all stages from the table (L1 / L2 resident: n_stage * C * 24 B) before its data arrives.
template <typename T, int VEC>
__global__ void __launch_bounds__(kBlock)
pointwise_cols_table_kernel(const T* __restrict__ x, T* __restrict__ y, int64_t n_vec, int n_lev, int C,
                            const atx_level_op* __restrict__ prog, const atx_level_op* __restrict__ vec_prog, int n_stage,
                            const uint8_t* __restrict__ point_mask, int in_place) {
    using V = Pack<T, VEC>;
    const int64_t vi = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (vi >= n_vec) return;
    int64_t row;
    int c;
    split_row_col(vi, n_vec, C, row, c);
    LevelOp<T> ops[kMaxStages];
    bool act = false, need_mask = false;
#pragma unroll
    for (int s = 0; s < kMaxStages; ++s) {
        if (s < n_stage) {
            ops[s] = load_level_op<T>(vec_prog, (int64_t)s * C + c);
            act = act || ops[s].op != ATX_OP_COPY || ops[s].use_mask != 0;
            need_mask = need_mask || ops[s].use_mask != 0;
        }
    }
    if (!act && in_place) return;  // untouched levels of an in-place call: nothing to move
    V v = pw_load<T, VEC>(x + vi * VEC);
    if (act) {
        const bool masked = (need_mask && point_mask) ? (point_mask[row] != 0) : false;
        apply_vector_ops<T, VEC>(ops, prog, n_stage, n_lev, c, v, masked);
    }
    pw_store<T, VEC>(y + vi * VEC, v);
}

// The same stacks when the program is UNIFORM over the levels (uniform_level_program: per stage one operator, or two pieces split
// on a vector boundary — rescale / convert / orog_to_z / clip / impute_nans / apply_mask over a whole stack, or "136 levels of t and
// one of orog"): the operators travel by value in the kernel arguments, so a lane's only memory traffic is its 16-byte vector (and
// one mask byte when a stage uses the point mask) — the launch shape and the instruction stream of atx_stream_copy plus a scalar
// branch per stage.  This is the shape whose speed does not move from box to box (atx_stream_copy: 2.33-2.35 ms for 137 float64
// levels of O1280 on every box of round 3, the chunked kernel 2.34-2.68 ms).  NT: non-temporal loads AND stores — nothing this
// kernel touches is touched again — measured 2.32 -> 2.22 ms f64 out of place, 2.43 -> 2.23 ms in place, f32 1.19 -> 1.13 and
// 1.24 -> 1.12 ms (0.80-0.81 of the peak, above the plain copy); with a point mask they cost 2-6 % instead (the mask bytes, shared
// by the ~35-69 lanes of a point, live in the same caches), so masked programs keep plain accesses; profiles/r03_pointwise_ab.log.
template <typename T, int VEC, bool TRANS, bool NT>
__global__ void __launch_bounds__(kBlock)
pointwise_cols_uniform_kernel(const T* __restrict__ x, T* __restrict__ y, int64_t n_vec, int C, int Cp, UniformOps<T> u,
                              const uint8_t* __restrict__ point_mask, int need_rc, int in_place, unsigned act_bits) {
    // Cp >= C: vector slots per row (pitch / VEC); n_vec = n_pts * Cp; slots beyond C are padding (need_rc is set when Cp > C)
    using V = Pack<T, VEC>;
    // One vector per lane (2-8 stream slower, tools/experiments/stream_shapes.hip).  The body keeps the shape it had when that
    // was a parameter: written out for scalars the compiler spends one more scalar register on it.
    constexpr int U = 1;
    const int64_t base = (int64_t)blockIdx.x * (kBlock * U) + threadIdx.x;
    V v[U];
    int c[U];
    bool masked[U], go[U];
#pragma unroll
    for (int k = 0; k < U; ++k) {
        const int64_t vi = base + (int64_t)k * kBlock;
        go[k] = vi < n_vec;
        c[k] = 0;
        masked[k] = false;
        if (go[k] && need_rc) {  // uniform: a two-piece stage or the point mask — the lane needs its (row, vector column)
            int64_t row;
            split_row_col(vi, n_vec, Cp, row, c[k]);
            if (c[k] >= C) go[k] = false;  // padding slot of a loose pitch
            if (in_place) {  // untouched columns of an in-place call: nothing to move.  `act_bits` (host-built): bit s = the first
                // piece of stage s does something, bit 4 + s = its second piece.  (Selecting between u.stage[s].op and u.second[s].op
                // here made the compiler select between their ADDRESSES and load per lane from the kernel-argument segment, two
                // dependent loads per stage ahead of the data load: apply_mask in place 3.51 ms instead of 2.45.)
                unsigned act = 0;
#pragma unroll
                for (int s = 0; s < kMaxUniform; ++s) act |= (c[k] >= u.split[s]) ? (act_bits >> (4 + s)) : (act_bits >> s);
                go[k] = go[k] && (act & 1u) != 0;
            }
            if (point_mask && go[k]) masked[k] = point_mask[row] != 0;  // a byte load per lane
        }
        if (go[k]) v[k] = NT ? pw_load_nt<T, VEC>(x + vi * VEC) : pw_load<T, VEC>(x + vi * VEC);
    }
#pragma unroll
    for (int k = 0; k < U; ++k) {
        if (!go[k]) continue;
        for (int s = 0; s < u.n_stage; ++s) {
            if (u.split[s] >= C) {  // scalar condition: one piece
                apply_level_op_vec<T, VEC, TRANS>(u.stage[s], v[k], masked[k]);
            } else {
                V other = v[k];
                apply_level_op_vec<T, VEC, TRANS>(u.stage[s], v[k], masked[k]);
                apply_level_op_vec<T, VEC, TRANS>(u.second[s], other, masked[k]);
                if (c[k] >= u.split[s]) v[k] = other;
            }
        }
        if (NT) pw_store_nt<T, VEC>(y + (base + (int64_t)k * kBlock) * VEC, v[k]);
        else pw_store<T, VEC>(y + (base + (int64_t)k * kBlock) * VEC, v[k]);
    }
}

// Programs made of RUNS of levels (RunOps: up to 4 per stage, boundaries anywhere — several variables sharing a column): the launch shape
// of the by-value kernel above — one 16-byte vector per lane, no loop, no shared memory, non-temporal accesses when no point mask is
// read — with every run's operator evaluated on the vector and the element's own kept.  Before round 4 such programs went through the
// per-level LDS kernel (0.70 / 0.75 of the peak).
template <typename T, int VEC, bool TRANS, bool NT>
__global__ void __launch_bounds__(kBlock)
pointwise_cols_runs_kernel(const T* __restrict__ x, T* __restrict__ y, int64_t n_vec, int C, int Cp, RunOps<T> runs,
                           const uint8_t* __restrict__ point_mask) {
    using V = Pack<T, VEC>;
    const int64_t vi = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (vi >= n_vec) return;
    int64_t row;
    int c;
    split_row_col(vi, n_vec, Cp, row, c);
    if (c >= C) return;  // padding slot of a loose pitch
    const bool masked = point_mask ? point_mask[row] != 0 : false;
    V v = NT ? pw_load_nt<T, VEC>(x + vi * VEC) : pw_load<T, VEC>(x + vi * VEC);
    apply_run_ops<T, VEC, TRANS>(runs, c, v, masked);
    if (NT) pw_store_nt<T, VEC>(y + vi * VEC, v);
    else pw_store<T, VEC>(y + vi * VEC, v);
}

// ONE stage whose 16-byte vectors each hold one operator KIND (the parameters may differ from level to level: a scale per level): one
// vector per lane, no loop, the parameters from the typed per-level part of the host-built table (level_tables_layout; two 16-byte
// loads and one code word per lane, L1 / L2 resident) — the launch shape of the by-value kernel.  Measured against the per-level LDS
// kernel, same box, interleaved (profiles/r03_per_level_programs.log): f64 +4 to +8 % (0.75-0.76 -> 0.78-0.80 on a fast box, 0.67-0.70 ->
// 0.71-0.75 on a slow one), f32 in place 0.70-0.74 -> 0.74-0.78, f32 out of place 0.81 -> 0.77 and f32 with the point mask 0.73 -> 0.69
// (those stay on the LDS kernel); two stages or vectors of mixed kinds lose 10-25 % here and stay there too.
template <typename T, int VEC, bool TRANS, bool NT>
__global__ void __launch_bounds__(kBlock)
pointwise_cols_typed_kernel(const T* __restrict__ x, T* __restrict__ y, int64_t n_vec, int C, const unsigned char* __restrict__ level_tables,
                            const uint8_t* __restrict__ point_mask, int in_place) {
    using V = Pack<T, VEC>;
    using OpWord = typename OpWordOf<VEC>::type;
    const int64_t vi = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (vi >= n_vec) return;
    int64_t row;
    int c;
    split_row_col(vi, n_vec, C, row, c);
    const int Lp = C * VEC;
    const T* tp0 = reinterpret_cast<const T*>(level_tables);
    const T* tp1 = tp0 + Lp;
    const uint8_t* tcd = reinterpret_cast<const uint8_t*>(tp1 + Lp);
    const unsigned code = *reinterpret_cast<const OpWord*>(tcd + c * VEC) & 0xffu;  // (the host checked: every level of the vector has this code)
    if (in_place && code == 0) return;  // untouched levels of an in-place call: nothing to move
    const V a = *reinterpret_cast<const V*>(tp0 + c * VEC);
    const V b = *reinterpret_cast<const V*>(tp1 + c * VEC);
    V v = NT ? pw_load_nt<T, VEC>(x + vi * VEC) : pw_load<T, VEC>(x + vi * VEC);
    if (code != 0) {
        const bool masked = ((code & 0x80u) && point_mask) ? (point_mask[row] != 0) : false;
        apply_level_op_params<T, VEC, TRANS>((int)(code & 0x7fu), (code & 0x80u) != 0, a, b, v, masked);
    }
    if (NT) pw_store_nt<T, VEC>(y + vi * VEC, v);
    else pw_store<T, VEC>(y + vi * VEC, v);
}

// In place with FEW active levels (1 of 137: one variable of a stack converted, a mask applied to one field): only the
// vector columns that hold an active level are visited — one (point, active column) item per lane, the column list by value in
// the kernel arguments.  The kernels above skip the loads of untouched columns too, but still walk all n_pts*C vector slots
// with 1 lane in 35 doing anything (1.53 ms for 1 of 137 levels on O1280, more than transforming the whole stack); here every
// lane has a 16-byte read-modify-write in flight.  The traffic is one 64/128-byte line per point and active column either way.
constexpr int kMaxActive = 16;
struct ActiveCols {
    int n;
    int col[kMaxActive];
};

template <typename T, int VEC>
__global__ void __launch_bounds__(kBlock)
pointwise_cols_sparse_kernel(T* __restrict__ y, int64_t n_items, int n_lev, int C, int64_t pitch, ActiveCols active,
                             const atx_level_op* __restrict__ prog, const atx_level_op* __restrict__ vec_prog, int n_stage,
                             const uint8_t* __restrict__ point_mask) {
    using V = Pack<T, VEC>;
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= n_items) return;
    const int64_t p = q / active.n;
    const int a = (int)(q - p * active.n);
    int c = active.col[0];
#pragma unroll
    for (int i = 1; i < kMaxActive; ++i) c = (a == i) ? active.col[i] : c;  // the list lives in scalar registers: select, do not index
    LevelOp<T> ops[kMaxStages];
    bool need_mask = false;
#pragma unroll
    for (int s = 0; s < kMaxStages; ++s) {
        if (s < n_stage) {
            ops[s] = load_level_op<T>(vec_prog, (int64_t)s * C + c);
            need_mask = need_mask || ops[s].use_mask != 0;
        }
    }
    T* at = y + p * pitch + (int64_t)c * VEC;
    V v = pw_load<T, VEC>(at);
    const bool masked = (need_mask && point_mask) ? (point_mask[p] != 0) : false;
    apply_vector_ops<T, VEC>(ops, prog, n_stage, n_lev, c, v, masked);
    pw_store<T, VEC>(at, v);
}

// ATX_FIELDS, round 3: one 16-byte vector per lane, no loop — grid.x = 1 KB-per-wave pieces of a field, grid.y = field.  The field's
// operators (uniform over the workgroup: scalar loads, scalar branches) stay in registers because the stage loop is fully unrolled
// — round 1's grid-stride kernel indexed ops[] with a run-time stage count, which put the array in scratch memory: 137 fields of O1280 ran at
// 0.40-0.44 of the HBM peak, two stages at 0.29 (tools/experiments/fields_pointwise.py).  The mask bytes of a vector's VEC points
// come as one 2- / 4-byte load (mask_vec: the mask base is aligned for it); non-temporal accesses when no mask is read.
// Measured on 137 fields of O1280 (profiles/r03_fields_pointwise.log; run-to-run noise ~3 %): requesting the data before the field's
// operators are known (out of place only — in place an untouched field must not be read) f32 0.78 -> 0.83, f64 neutral; two vectors
// per lane f64 0.75-0.77 -> 0.78-0.80 (and an in-place call that skips two fields in three 1.25 -> 0.95 ms), f32 in place 0.78 -> 0.75.
template <typename T>
constexpr int fields_vectors_per_lane() {  // kBlock apart
    return sizeof(T) == 4 ? 1 : 2;
}
template <typename T, int VEC, bool TRANS, bool NT>
__global__ void __launch_bounds__(kBlock)
pointwise_fields_rows_kernel(const T* __restrict__ x, T* __restrict__ y, int64_t n_pts, int n_lev,
                             int64_t x_pitch, int64_t y_pitch, const atx_level_op* __restrict__ prog, int n_stage,
                             const uint8_t* __restrict__ point_mask, int in_place, int mask_vec) {
    using V = Pack<T, VEC>;
    using MaskWord = typename OpWordOf<VEC>::type;
    constexpr int U = fields_vectors_per_lane<T>();
    const int l = blockIdx.y;
    const T* xs = x + (int64_t)l * x_pitch;
    T* ys = y + (int64_t)l * y_pitch;
    const int64_t n_vec = n_pts / VEC;
    const int64_t base = (int64_t)blockIdx.x * (kBlock * U) + threadIdx.x;
    V v[U];
    const bool early = !in_place;
    if (early) {
#pragma unroll
        for (int k = 0; k < U; ++k)
            if (base + k * kBlock < n_vec) v[k] = NT ? pw_load_nt<T, VEC>(xs + (base + k * kBlock) * VEC) : pw_load<T, VEC>(xs + (base + k * kBlock) * VEC);
    }
    LevelOp<T> ops[8];
    bool act = false, need_mask = false;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        ops[s].op = ATX_OP_COPY;
        ops[s].use_mask = 0;
        ops[s].p0 = ops[s].p1 = T(0);
        if (s < n_stage) {
            ops[s] = load_level_op<T>(prog, (int64_t)s * n_lev + l);
            act = act || ops[s].op != ATX_OP_COPY || ops[s].use_mask != 0;
            need_mask = need_mask || ops[s].use_mask != 0;
        }
    }
    if (!act && in_place) return;  // untouched field: identity (R: filter.py:193-194)
    if (!early) {
#pragma unroll
        for (int k = 0; k < U; ++k)
            if (base + k * kBlock < n_vec) v[k] = NT ? pw_load_nt<T, VEC>(xs + (base + k * kBlock) * VEC) : pw_load<T, VEC>(xs + (base + k * kBlock) * VEC);
    }
#pragma unroll
    for (int k = 0; k < U; ++k) {
        const int64_t vi = base + k * kBlock;
        if (vi >= n_vec) continue;
        if (act) {
            unsigned mbits = 0;  // byte e: the mask of point vi * VEC + e
            if (need_mask && point_mask) {
                if (mask_vec) {
                    mbits = *reinterpret_cast<const MaskWord*>(point_mask + vi * VEC);
                } else {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) mbits |= (unsigned)point_mask[vi * VEC + e] << (8 * e);
                }
            }
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                if (s < n_stage) {
                    LevelOp<T> o = ops[s];
                    const bool use_mask = o.use_mask != 0;
                    o.use_mask = 0;
                    apply_level_op_vec<T, VEC, TRANS>(o, v[k], false);
                    if (use_mask) {
#pragma unroll
                        for (int e = 0; e < VEC; ++e)
                            if ((mbits >> (8 * e)) & 0xffu) v[k].v[e] = quiet_nan<T>();
                    }
                }
            }
        }
        if (NT) pw_store_nt<T, VEC>(ys + vi * VEC, v[k]);
        else pw_store<T, VEC>(ys + vi * VEC, v[k]);
    }
    // tail points (n_pts % VEC) by the first lanes of block 0
    if (VEC > 1 && blockIdx.x == 0) {
        const int64_t i = n_vec * VEC + threadIdx.x;
        if (threadIdx.x < VEC && i < n_pts) {
            T t = xs[i];
            if (act) {
                const bool masked = point_mask ? (point_mask[i] != 0) : false;
#pragma unroll
                for (int s = 0; s < 8; ++s)
                    if (s < n_stage) t = apply_level_op<T, TRANS>(ops[s], t, masked);
            }
            ys[i] = t;
        }
    }
}

// ---- dispatch -----------------------------------------------------------------------------------------------------------------

// (with_flag: atx_common.hpp)
template <typename F>
static void with_trans_nt(bool trans, bool nt, F&& f) {
    with_flag(trans, [&](auto tr) { with_flag(nt, [&](auto n) { f(tr, n); }); });
}

// Does vector column c (levels c*vec .. c*vec+vec-1) hold a level that some stage does not plainly COPY?
static bool vector_column_active(const atx_level_op* host_prog, int n_stage, int n_lev, int c, int vec) {
    for (int s = 0; s < n_stage; ++s)
        for (int l = c * vec; l < n_lev && l < (c + 1) * vec; ++l) {
            const atx_level_op& o = host_prog[(int64_t)s * n_lev + l];
            if (o.op != ATX_OP_COPY || o.use_mask != 0) return true;
        }
    return false;
}

// One ATX_COLUMNS call and what every route wants to know about it.
template <typename T>
struct ColumnsCall {
    static constexpr int VEC = Vec16<T>::N;
    const T* x;
    T* y;
    int64_t n_pts;
    int n_lev;
    int64_t xp, yp;
    const atx_level_op *prog, *vec_prog, *host_prog;
    int n_stage;
    const uint8_t* mask;
    hipStream_t st;
    int in_place;
    bool wide;  // 16-byte vectors: bases and pitches aligned, the last (partial) vector of a row inside both pitches
    int C;      // columns of a row: vectors when wide, levels otherwise
    // One run of vector slots — a tight pitch, or (round 3) equal loose pitches (columns aligned to 128 bytes, a spare vector): the
    // no-loop and chunked kernels walk the Cp = pitch / VEC slots of a row and leave the padding slots alone (the row-chunk kernel:
    // 0.51-0.57 f32, 0.69 f64 on such stacks).  Cp, n_vec and one_launch mean something only when `slots` is set.
    bool slots, tight;
    int Cp;
    int64_t n_vec;    // n_pts * Cp
    bool one_launch;  // one vector per lane fits the grid

    bool transcendental() const { return program_has_transcendental(host_prog, n_stage, n_lev); }
    dim3 vector_grid() const { return dim3((unsigned)((n_vec + kBlock - 1) / kBlock)); }
    dim3 chunk_grid() const {  // contiguous runs of `per` chunks of kBlock * kPwUnroll vectors: no workgroup without work
        const int64_t n_chunks = (n_vec + (int64_t)kBlock * kPwUnroll - 1) / ((int64_t)kBlock * kPwUnroll);
        const int64_t blocks = n_chunks > kStreamGrid ? kStreamGrid : n_chunks;
        const int64_t per = (n_chunks + blocks - 1) / blocks;
        return dim3((unsigned)((n_chunks + per - 1) / per));
    }
};

// A route launches and returns a status (ATX_OK, an error, ATX_SPLIT_PROGRAM), or declines with no value.
using Routed = std::optional<int>;

// In place with few active levels: visit their columns only.
template <typename T>
static Routed route_sparse(const ColumnsCall<T>& k) {
    constexpr int VEC = ColumnsCall<T>::VEC;
    if (!(k.in_place && k.wide && k.host_prog && k.vec_prog)) return std::nullopt;
    ActiveCols active{};
    for (int c = 0; c < k.C; ++c) {
        if (!vector_column_active(k.host_prog, k.n_stage, k.n_lev, c, VEC)) continue;
        if (active.n == kMaxActive) return std::nullopt;
        active.col[active.n++] = c;
    }
    if (active.n == 0) return ATX_OK;  // nothing to do at all
    if (3 * active.n > k.C) return std::nullopt;
    for (int i = active.n; i < kMaxActive; ++i) active.col[i] = active.col[0];
    const int64_t n_items = k.n_pts * active.n;
    const int64_t blocks = (n_items + kBlock - 1) / kBlock;
    ATX_REQUIRE(blocks <= 0x7fffffffll, ATX_ENOTIMPL, "pointwise: %lld items exceed one launch", (long long)n_items);
    g_last_route = "sparse";
    hipLaunchKernelGGL((pointwise_cols_sparse_kernel<T, VEC>), dim3((unsigned)blocks), dim3(kBlock), 0, k.st, k.y, n_items, k.n_lev, k.C, k.yp,
                       active, k.prog, k.vec_prog, k.n_stage, k.mask);
    ATX_LAUNCH_CHECK("pointwise_stack_sparse");
    return ATX_OK;
}

// Programs uniform over the levels: operators by value, one vector per lane, no loop.  Non-temporal unless the point mask is read
// (with it: 2-6 % slower, profiles/r04_apply_mask_experiment.log), programs with exp / log included.
template <typename T>
static Routed route_uniform(const ColumnsCall<T>& k) {
    constexpr int VEC = ColumnsCall<T>::VEC;
    UniformOps<T> uni{};
    if (!(k.slots && k.one_launch && uniform_level_program<T>(k.host_prog, k.n_stage, k.mask != nullptr, k.n_lev, VEC, uni))) return std::nullopt;
    bool two_pieces = false, uses_mask = false;
    unsigned act_bits = 0;
    for (int s = 0; s < k.n_stage; ++s) {
        two_pieces = two_pieces || uni.split[s] < k.C;
        uses_mask = uses_mask || uni.stage[s].use_mask || uni.second[s].use_mask;
        if (uni.stage[s].op != ATX_OP_COPY || uni.stage[s].use_mask) act_bits |= 1u << s;
        if (uni.second[s].op != ATX_OP_COPY || uni.second[s].use_mask) act_bits |= 1u << (4 + s);
    }
    const int need_rc = (two_pieces || (uses_mask && k.mask) || !k.tight) ? 1 : 0;
    const bool nt = !(uses_mask && k.mask);
    g_last_route = "uniform";
    with_trans_nt(k.transcendental(), nt, [&](auto tr, auto n) {
        hipLaunchKernelGGL((pointwise_cols_uniform_kernel<T, VEC, decltype(tr)::value, decltype(n)::value>), k.vector_grid(), dim3(kBlock), 0, k.st,
                           k.x, k.y, k.n_vec, k.C, k.Cp, uni, uses_mask ? k.mask : nullptr, need_rc, k.in_place, act_bits);
    });
    ATX_LAUNCH_CHECK("pointwise_stack_uniform");
    return ATX_OK;
}

// Runs of levels with boundaries anywhere (several variables in one column), out of place or in place: by value as well.
// Measured against the routes below (tools/experiments/runs_probe.py, profiles/r04_runs_probe.log): evaluating every run's operator and
// selecting costs a streaming kernel more than it saves — one stage of 3 runs 0.72 / 0.67 (f32 / f64) here against 0.76 / 0.72 on the
// table and per-level kernels — except for float32 programs of two or more stages, which those kernels run at 0.52-0.58 and this one
// at 0.65-0.66.  So only they take it.
template <typename T>
static Routed route_runs(const ColumnsCall<T>& k) {
    constexpr int VEC = ColumnsCall<T>::VEC;
    RunOps<T> runs{};
    if (!(k.slots && sizeof(T) == 4 && k.n_stage >= 2 && k.one_launch && runs_level_program<T>(k.host_prog, k.n_stage, k.mask != nullptr, k.n_lev, runs)))
        return std::nullopt;
    bool uses_mask = false;
    for (int s = 0; s < k.n_stage; ++s)
        for (int r = 0; r < runs.n_run[s]; ++r) uses_mask = uses_mask || runs.op[s][r].use_mask != 0;
    const bool nt = !(uses_mask && k.mask);
    g_last_route = "runs";
    with_trans_nt(k.transcendental(), nt, [&](auto tr, auto n) {
        hipLaunchKernelGGL((pointwise_cols_runs_kernel<T, VEC, decltype(tr)::value, decltype(n)::value>), k.vector_grid(), dim3(kBlock), 0, k.st,
                           k.x, k.y, k.n_vec, k.C, k.Cp, runs, uses_mask ? k.mask : nullptr);
    });
    ATX_LAUNCH_CHECK("pointwise_stack_runs");
    return ATX_OK;
}

// Operators differing from level to level.  Measured (137 levels of O1280, profiles/r03_pointwise_ab.log): the table kernel (one
// vector per lane, no loop, operators from the host-built per-vector table) wins for one-stage f32 programs without a mask, out of
// place (1.21 ms both) AND in place (1.22 vs 1.36 ms chunked); it loses in f64 (2.48 vs 2.37 ms), with two stages (f32 1.56 vs 1.28,
// f64 3.38 vs 2.58 ms: 24-32 B of operators per stage and vector) and with a point mask in f64 (2.74 vs 2.43 ms).
template <typename T>
static Routed route_table(const ColumnsCall<T>& k) {
    constexpr int VEC = ColumnsCall<T>::VEC;
    if (!(k.slots && k.tight && k.vec_prog && !k.mask && sizeof(T) == 4 && k.n_stage == 1 && k.one_launch &&
          !program_has_mixed_vectors<T>(k.host_prog, k.n_stage, k.n_lev, VEC)))  // (mixed vectors: the chunked kernel serves them better)
        return std::nullopt;
    g_last_route = "table";
    hipLaunchKernelGGL((pointwise_cols_table_kernel<T, VEC>), k.vector_grid(), dim3(kBlock), 0, k.st, k.x, k.y, k.n_vec, k.n_lev, k.C, k.prog,
                       k.vec_prog, k.n_stage, k.mask, k.in_place);
    ATX_LAUNCH_CHECK("pointwise_stack");
    return ATX_OK;
}

// One stage, one operator kind per vector (a scale per level), float64 or in place: the no-loop kernel on the typed per-level part
// of vec_prog (everything else measured faster on the per-level LDS kernel below, profiles/r03_per_level_programs.log).
template <typename T>
static Routed route_typed(const ColumnsCall<T>& k) {
    constexpr int VEC = ColumnsCall<T>::VEC;
    if (!(k.slots && k.tight && k.n_stage == 1 && (sizeof(T) == 8 || k.in_place) && k.vec_prog && aligned16(k.vec_prog) && k.host_prog && k.one_launch))
        return std::nullopt;
    bool one_kind = true, uses_mask = false;
    for (int l0 = 0; l0 < k.n_lev && one_kind; l0 += VEC)
        for (int l = l0; l < k.n_lev && l < l0 + VEC; ++l) {
            one_kind = one_kind && k.host_prog[l].op == k.host_prog[l0].op && (k.host_prog[l].use_mask != 0) == (k.host_prog[l0].use_mask != 0);
            uses_mask = uses_mask || k.host_prog[l].use_mask != 0;
        }
    if (!(one_kind && (sizeof(T) == 8 || !(uses_mask && k.mask)))) return std::nullopt;  // (float32 with the point mask: 0.69 here against 0.71-0.75)
    const unsigned char* level_tables = reinterpret_cast<const unsigned char*>(k.vec_prog) +
                                        level_tables_layout(1, k.n_lev, sizeof(T) == 4 ? ATX_F32 : ATX_F64).levels_offset;
    const bool nt = !(uses_mask && k.mask);
    g_last_route = "typed";
    with_trans_nt(k.transcendental(), nt, [&](auto tr, auto n) {
        hipLaunchKernelGGL((pointwise_cols_typed_kernel<T, VEC, decltype(tr)::value, decltype(n)::value>), k.vector_grid(), dim3(kBlock), 0, k.st,
                           k.x, k.y, k.n_vec, k.C, level_tables, uses_mask ? k.mask : nullptr, k.in_place);
    });
    ATX_LAUNCH_CHECK("pointwise_stack_typed");
    return ATX_OK;
}

// Everything else on tight pitches whose per-level tables fit the LDS: the chunked sweep.  (Loose pitches measured slower here than
// on the row-chunk kernel — f64 0.57 against 0.69 — so only the by-value kernels take them; tools/experiments/loose_pitch.py.)
// Non-temporal for float32 programs the host can see, when every vector is touched; never with exp / log.
template <typename T>
static Routed route_levels(const ColumnsCall<T>& k) {
    constexpr int VEC = ColumnsCall<T>::VEC;
    if (!(k.slots && k.tight)) return std::nullopt;
    const size_t lds_levels = level_tables_lds_bytes<T>(k.n_stage, k.C, VEC) + (size_t)k.C;
    if (lds_levels > 64 * 1024) return std::nullopt;
    bool nt = sizeof(T) == 4 && k.host_prog != nullptr;
    if (nt && k.in_place)  // every vector must be touched
        for (int c = 0; c < k.C && nt; ++c) nt = vector_column_active(k.host_prog, k.n_stage, k.n_lev, c, VEC);
    auto launch = [&](auto tr, auto n) {
        hipLaunchKernelGGL((pointwise_cols_levels_kernel<T, VEC, decltype(tr)::value, decltype(n)::value>), k.chunk_grid(), dim3(kBlock), lds_levels, k.st,
                           k.x, k.y, k.n_pts, k.n_lev, k.C, k.Cp, k.prog, k.n_stage, k.mask, k.in_place);
    };
    g_last_route = "levels";
    if (k.transcendental()) launch(std::true_type{}, std::false_type{});
    else with_flag(nt, [&](auto n) { launch(std::false_type{}, n); });
    ATX_LAUNCH_CHECK("pointwise_stack_levels");
    return ATX_OK;
}

// Very tall stacks: round 2's chunked kernel, whose per-VECTOR table is smaller (tight pitches only).
template <typename T>
static Routed route_flat(const ColumnsCall<T>& k) {
    constexpr int VEC = ColumnsCall<T>::VEC;
    if (!(k.slots && k.tight)) return std::nullopt;
    const size_t lds_flat = (size_t)k.n_stage * k.C * sizeof(LevelOp<T>) + (size_t)k.C;
    if (lds_flat > 64 * 1024 && k.n_stage > 1) return ATX_SPLIT_PROGRAM;  // the entry point runs the stages in two halves
    ATX_REQUIRE(lds_flat <= 64 * 1024, ATX_ENOTIMPL, "pointwise: one stage over %d levels needs %zu B of LDS", k.n_lev, lds_flat);
    g_last_route = "flat";
    with_flag(k.transcendental(), [&](auto tr) {  // no exp / log anywhere: the low-register instantiation (8 instead of 4 waves per SIMD in float64)
        hipLaunchKernelGGL((pointwise_cols_flat_kernel<T, VEC, decltype(tr)::value>), k.chunk_grid(), dim3(kBlock), lds_flat, k.st, k.x, k.y, k.n_pts,
                           k.n_lev, k.C, k.prog, k.n_stage, k.mask, k.in_place);
    });
    ATX_LAUNCH_CHECK("pointwise_stack");
    return ATX_OK;
}

// Any pitches, any alignment: contiguous chunks of rows.
template <typename T>
static Routed route_row_chunk(const ColumnsCall<T>& k) {
    constexpr int VEC = ColumnsCall<T>::VEC;
    const size_t lds_rows = level_tables_lds_bytes<T>(k.n_stage, k.C, k.wide ? VEC : 1);
    if (lds_rows > 64 * 1024 && k.n_stage > 1) return ATX_SPLIT_PROGRAM;  // the entry point runs the stages in two halves
    ATX_REQUIRE(lds_rows <= 64 * 1024, ATX_ENOTIMPL, "pointwise: one stage over %d levels needs %zu B of LDS", k.n_lev, lds_rows);
    const int Cg = k.C < kBlock ? k.C : kBlock;
    const int chunk = (kBlock / Cg) * kPwUnroll;  // rows one workgroup moves per iteration
    const unsigned blocks = grid_for(k.n_pts, chunk, kStreamGrid);
    g_last_route = k.wide ? "row_chunk" : "row_chunk_scalar";
    if (k.wide)
        hipLaunchKernelGGL((pointwise_cols_kernel<T, VEC>), dim3((unsigned)blocks), dim3(kBlock), lds_rows, k.st, k.x, k.y, k.n_pts, k.n_lev, k.C, k.xp,
                           k.yp, k.prog, k.n_stage, k.mask, k.in_place);
    else
        hipLaunchKernelGGL((pointwise_cols_kernel<T, 1>), dim3((unsigned)blocks), dim3(kBlock), lds_rows, k.st, k.x, k.y, k.n_pts, k.n_lev, k.C, k.xp,
                           k.yp, k.prog, k.n_stage, k.mask, k.in_place);
    ATX_LAUNCH_CHECK("pointwise_stack");
    return ATX_OK;
}

template <typename T>
static int pointwise_columns(const void* x_, void* y_, int64_t n_pts, int n_lev, int64_t xp, int64_t yp, const atx_level_op* prog,
                             const atx_level_op* vec_prog, const atx_level_op* host_prog, int n_stage, const uint8_t* mask, hipStream_t st) {
    constexpr int VEC = Vec16<T>::N;
    ColumnsCall<T> k{static_cast<const T*>(x_), static_cast<T*>(y_), n_pts, n_lev, xp, yp, prog, vec_prog, host_prog, n_stage, mask, st};
    k.in_place = (x_ == y_ && xp == yp) ? 1 : 0;
    const int64_t covered = ((int64_t)(n_lev + VEC - 1) / VEC) * VEC;
    k.wide = aligned16(x_) && aligned16(y_) && (xp % VEC == 0) && (yp % VEC == 0) && covered <= xp && covered <= yp;
    k.C = k.wide ? (n_lev + VEC - 1) / VEC : n_lev;
    k.slots = k.wide && yp == xp && xp % VEC == 0 && xp / VEC <= 0x7fffffffll / 2;
    k.tight = xp == (int64_t)k.C * VEC;
    k.Cp = k.slots ? (int)(xp / VEC) : 0;
    k.n_vec = n_pts * k.Cp;
    k.one_launch = (k.n_vec + kBlock - 1) / kBlock <= 0x7fffffffll;
    Routed (*const routes[])(const ColumnsCall<T>&) = {route_sparse<T>, route_uniform<T>, route_runs<T>,  route_table<T>,
                                                     route_typed<T>,  route_levels<T>,  route_flat<T>};
    for (auto route : routes) {
        if (const Routed rc = route(k)) return *rc;
    }
    return *route_row_chunk<T>(k);
}

template <typename T>
static int pointwise_fields(const void* x_, void* y_, int64_t n_pts, int n_lev, int64_t xp, int64_t yp, const atx_level_op* prog,
                            const atx_level_op* host_prog, int n_stage, const uint8_t* mask, hipStream_t st) {
    const T* x = static_cast<const T*>(x_);
    T* y = static_cast<T*>(y_);
    const int in_place = (x_ == y_ && xp == yp) ? 1 : 0;
    constexpr int VEC = Vec16<T>::N;
    const bool vec_ok = aligned16(x_) && aligned16(y_) && (xp % VEC == 0) && (yp % VEC == 0);
    ATX_REQUIRE(n_lev <= 65535, ATX_ENOTIMPL, "pointwise: n_lev=%d exceeds grid.y", n_lev);
    const int vec = vec_ok ? VEC : 1;
    const int64_t per_block = (int64_t)kBlock * fields_vectors_per_lane<T>();
    const int64_t gx_rows = (std::max<int64_t>(n_pts / vec, 1) + per_block - 1) / per_block;
    ATX_REQUIRE(gx_rows <= 0x7fffffffll, ATX_ENOTIMPL, "pointwise: %lld points per field exceed one launch", (long long)n_pts);
    bool uses_mask = mask != nullptr;  // unknown program: assume it reads the mask it was given
    if (host_prog && mask) {
        uses_mask = false;
        for (int64_t i = 0; i < (int64_t)n_stage * n_lev; ++i) uses_mask = uses_mask || host_prog[i].use_mask != 0;
    }
    const bool trans = program_has_transcendental(host_prog, n_stage, n_lev);
    const int mask_vec = (reinterpret_cast<uintptr_t>(mask) % (uintptr_t)vec) == 0 ? 1 : 0;
    const dim3 grid((unsigned)gx_rows, (unsigned)n_lev);
    g_last_route = vec_ok ? "fields" : "fields_scalar";
    if (vec_ok)  // non-temporal when no mask is read
        with_trans_nt(trans, !uses_mask, [&](auto tr, auto n) {
            hipLaunchKernelGGL((pointwise_fields_rows_kernel<T, VEC, decltype(tr)::value, decltype(n)::value>), grid, dim3(kBlock), 0, st, x, y, n_pts,
                               n_lev, xp, yp, prog, n_stage, mask, in_place, mask_vec);
        });
    else
        with_flag(trans, [&](auto tr) {
            hipLaunchKernelGGL((pointwise_fields_rows_kernel<T, 1, decltype(tr)::value, false>), grid, dim3(kBlock), 0, st, x, y, n_pts, n_lev, xp, yp,
                               prog, n_stage, mask, in_place, mask_vec);
        });
    ATX_LAUNCH_CHECK("pointwise_stack_fields");
    return ATX_OK;
}

}  // namespace atx

using namespace atx;

extern "C" int atx_pointwise_stack(const void* x, void* y, int64_t n_pts, int64_t n_lev, int64_t x_pitch,
                                   int64_t y_pitch, int dtype, int layout, const atx_level_op* prog,
                                   const atx_level_op* vec_prog, const atx_level_op* host_prog, int32_t n_stage,
                                   const uint8_t* point_mask, void* stream) {
    g_last_route = "none";  // until a route launches (atx_last_route)
    ATX_REQUIRE(prog && ((x && y) || n_pts == 0), ATX_EINVAL, "atx_pointwise_stack: null pointer");  // (an empty stack may have no storage)
    ATX_REQUIRE(dtype == ATX_F32 || dtype == ATX_F64, ATX_EINVAL, "atx_pointwise_stack: bad dtype %d", dtype);
    ATX_REQUIRE(layout == ATX_COLUMNS || layout == ATX_FIELDS, ATX_EINVAL, "atx_pointwise_stack: bad layout %d", layout);
    ATX_REQUIRE(n_pts >= 0 && n_lev > 0 && n_lev <= 65535, ATX_EINVAL, "atx_pointwise_stack: bad sizes n_pts=%lld n_lev=%lld",
                (long long)n_pts, (long long)n_lev);
    ATX_REQUIRE(n_stage >= 1 && n_stage <= 8, ATX_EINVAL, "atx_pointwise_stack: n_stage=%d outside [1, 8]", n_stage);
    const int64_t need = layout == ATX_COLUMNS ? n_lev : n_pts;
    ATX_REQUIRE(x_pitch >= need && y_pitch >= need, ATX_ESHAPE, "atx_pointwise_stack: pitch (%lld, %lld) < %lld",
                (long long)x_pitch, (long long)y_pitch, (long long)need);
    if (n_pts == 0) return ATX_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int L = (int)n_lev;
    int rc;
    if (layout == ATX_COLUMNS)
        rc = dtype == ATX_F32 ? pointwise_columns<float>(x, y, n_pts, L, x_pitch, y_pitch, prog, vec_prog, host_prog, n_stage, point_mask, s)
                              : pointwise_columns<double>(x, y, n_pts, L, x_pitch, y_pitch, prog, vec_prog, host_prog, n_stage, point_mask, s);
    else
        rc = dtype == ATX_F32 ? pointwise_fields<float>(x, y, n_pts, L, x_pitch, y_pitch, prog, host_prog, n_stage, point_mask, s)
                              : pointwise_fields<double>(x, y, n_pts, L, x_pitch, y_pitch, prog, host_prog, n_stage, point_mask, s);
    if (rc != ATX_SPLIT_PROGRAM) return rc;
    // The program's per-level tables exceed the LDS budget (n_stage > 1 here): stages compose, y = s_{n-1}( ... s_0(x)), so the first
    // half goes x -> y and the second half y -> y in place — same statements in the same order, same bits.  vec_prog is laid out for the
    // whole program and does not travel with a part of it.
    const int32_t first = n_stage / 2;
    const int rc_first = atx_pointwise_stack(x, y, n_pts, n_lev, x_pitch, y_pitch, dtype, layout, prog, nullptr, host_prog, first, point_mask, stream);
    if (rc_first != ATX_OK) return rc_first;
    return atx_pointwise_stack(y, y, n_pts, n_lev, y_pitch, y_pitch, dtype, layout, prog + (int64_t)first * n_lev, nullptr,
                               host_prog ? host_prog + (int64_t)first * n_lev : nullptr, n_stage - first, point_mask, stream);
}
