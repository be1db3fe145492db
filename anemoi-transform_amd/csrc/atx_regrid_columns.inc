// The gather on ATX_COLUMNS stacks (DESIGN.md §3): three kernels, their launchers, and the ladder that picks a compile-time k.
//  * regrid_cols_ell_direct_kernel — fixed k in {1..8, 12, 16} (padded ragged rows from 3): one (target, 16-byte vector) item per
//    lane, no shared memory, no barrier, no loop; consecutive lanes read consecutive 16 B of one source column and write consecutive
//    16 B of the output.  The headline kernel.  It also takes the fused per-level program when the operators can reach it without a
//    per-workgroup set-up: by value (uniform / runs) or through the host-built per-vector table.
//  * regrid_cols_ell_kernel — the TILED form: a workgroup owns a tile of consecutive targets, stages their indices / weights (and
//    the operator tables of an epilogue) in LDS once, then sweeps the flattened (target, vector) items with up to 4 in flight per
//    lane.  Every other k, every other epilogue, and anything under atx_set_tuning(tile > 0).
//  * regrid_cols_csr_kernel — general CSR rows from a staged slice of the CSR arrays.
// Workgroups are dealt to the XCDs in contiguous ranges (xcd_tile), so that neighbouring targets that share source columns share
// an L2 — or, for long rows in natural order, in stripes (xcd_stripe).  Several stacks of one shape share a launch (grid.y = stack).
// Included by atx_regrid_typed.inc; the helpers shared with the fields piece are in atx_regrid_decl.hpp.

namespace atx {

// The measured winners of rounds 1-4, frozen (HISTORY.md, "The gather kernels' A/B knobs, frozen").
constexpr int kEllBlock = 256;  // lanes per workgroup of the fixed-k kernels: 64 / 128 / 512 / 1024 reach the same plateau (profiles/r01_ab_block_sizes.log, r03_ell_block_sweep.log)
constexpr int kUnroll = 4;      // items in flight per lane of the tiled kernel: 2 and 8 gain nothing (profiles/r01_ab_variants.log)
constexpr unsigned kLongRowStripe = 64;   // direct kernel, K >= 5 in natural order: workgroups per XCD in turn (see launch_cols_ell)
constexpr int kCsrStripe = 16;            // CSR kernel in natural order: tiles per XCD in turn ...
constexpr double kCsrStripeMinMean = 8.0; // ... from this mean row length (see launch_cols_csr)

// ---------------------------------------------------------------------------------
// ATX_COLUMNS, fixed k (ELL), tiled.  K > 0: compile-time k; K == 0: runtime k.
// ---------------------------------------------------------------------------------
// Up to kMaxBatch stacks of identical shape share one launch (several variables or time steps on the same grid
// pair, or the N source stacks of a target-sharded multi-GPU step): blockIdx.y selects the stack, so the launch gaps
// and per-launch tails of a stack-by-stack loop disappear.  The pointers travel by value in the kernel arguments.

template <typename T, int VEC, int K, bool WEIGHTED, bool EPI, bool PAD>
__global__ void __launch_bounds__(kEllBlock)
regrid_cols_ell_kernel(EllBatch batch,
                       const int32_t* __restrict__ idx, const T* __restrict__ w,
                       int64_t n_tgt, int k_rt, int n_lev, int C,
                       int64_t src_pitch, int64_t out_pitch, int tile, unsigned n_tiles,
                       const atx_level_op* __restrict__ prog, int n_stage,
                       const uint8_t* __restrict__ tgt_mask, const int32_t* __restrict__ tgt_rows) {
    using V = Pack<T, VEC>;
    // items in flight per lane: the epilogue variant trades half of them for registers (its operator
    // dispatch would otherwise push the kernel from 5 to 2-4 waves per SIMD; 2 vs 4 in flight costs ~1 %)
    constexpr int kU = EPI ? 2 : kUnroll;
    extern __shared__ __align__(16) unsigned char smem[];
    const int k = K > 0 ? K : k_rt;
    // LDS carve: weights (widest type first), indices, then the level program
    T* w_s = reinterpret_cast<T*>(smem);
    int32_t* idx_s = reinterpret_cast<int32_t*>(w_s + (WEIGHTED ? (size_t)tile * k : 0));
    unsigned char* prog_s = smem + (((WEIGHTED ? (size_t)tile * k * sizeof(T) : 0) + (size_t)tile * k * sizeof(int32_t) + 15) & ~size_t(15));

    const unsigned tile_id = xcd_tile(blockIdx.x, n_tiles);  // plain blockIdx.x: -3 % (profiles/r01_ab_variants.log, no_xcd)
    const int64_t t0 = (int64_t)tile_id * tile;
    const int nt = (int)min((int64_t)tile, n_tgt - t0);
    const int tid = threadIdx.x;

    for (int i = tid; i < nt * k; i += kEllBlock) {
        idx_s[i] = load_once(idx + t0 * k + i);
        if (WEIGHTED) w_s[i] = load_once(w + t0 * k + i);
    }
    LevelTablesLds<T> tab{};  // the operators of every level (atx_common.hpp)
    if (EPI) tab = build_level_tables<T, VEC>(prog, prog_s, n_stage, n_lev, C, tid, kEllBlock);
    __syncthreads();

    const int items = nt * C;
    const int dt = kEllBlock / C;
    const int dc = kEllBlock - dt * C;

    // stacks of a batch: grid.y keeps workgroups short — measured 0.45 ms per 8-stack step on a 1/8 target shard against
    // 0.51 ms for a loop over the stacks inside the workgroup (which stages the tile once but runs 8x longer) and
    // 0.50-0.52 ms for 8 separate launches (profiles/r01_shard_balance.log)
    const T* __restrict__ src = static_cast<const T*>(batch.src[blockIdx.y]);
    T* __restrict__ out = static_cast<T*>(batch.out[blockIdx.y]);
    int t = tid / C;
    int c = tid - t * C;

    for (int q = tid; q < items; q += kEllBlock * kU) {
        int tt[kU], cc[kU];
        bool ok[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            ok[u] = (q + u * kEllBlock) < items;
            tt[u] = ok[u] ? t : 0;
            cc[u] = ok[u] ? c : 0;
            t += dt;
            c += dc;
            if (c >= C) { c -= C; ++t; }
        }

        V acc[kU];
        if (K > 0) {
            // all K*kU loads are independent: issue them before any arithmetic
            V v[kU][K > 0 ? K : 1];
#pragma unroll
            for (int u = 0; u < kU; ++u) {
#pragma unroll
                for (int j = 0; j < (K > 0 ? K : 1); ++j) {
                    int64_t p = idx_s[tt[u] * K + j];
                    // absent entry of a padded row: load anything valid, skipped below (predicating the load instead was
                    // measured 20 % slower: the branch breaks up the batch of independent loads)
                    if (PAD && p < 0) p = 0;
                    v[u][j] = load_src<T, VEC>(src + p * src_pitch + (int64_t)cc[u] * VEC);
                }
            }
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                if (WEIGHTED) {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) acc[u].v[e] = T(0);
#pragma unroll
                    for (int j = 0; j < (K > 0 ? K : 1); ++j) {
                        const T wj = w_s[tt[u] * K + j];
                        if (!PAD || idx_s[tt[u] * K + j] >= 0) {
#pragma unroll
                            for (int e = 0; e < VEC; ++e) acc[u].v[e] = acc[u].v[e] + wj * v[u][j].v[e];
                        }
                    }
                } else {
                    acc[u] = v[u][0];
                }
            }
        } else {
#pragma unroll
            for (int u = 0; u < kU; ++u) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc[u].v[e] = T(0);
                const int base = tt[u] * k;
                int j = 0;
                for (; j + 2 <= k; j += 2) {
                    const int64_t pa = idx_s[base + j], pb = idx_s[base + j + 1];
                    const V va = *reinterpret_cast<const V*>(src + ((PAD && pa < 0) ? 0 : pa) * src_pitch + (int64_t)cc[u] * VEC);
                    const V vb = *reinterpret_cast<const V*>(src + ((PAD && pb < 0) ? 0 : pb) * src_pitch + (int64_t)cc[u] * VEC);
                    const T wa = WEIGHTED ? w_s[base + j] : T(1), wb = WEIGHTED ? w_s[base + j + 1] : T(1);
#pragma unroll
                    for (int e = 0; e < VEC; ++e) {
                        if (!PAD || pa >= 0) acc[u].v[e] = acc[u].v[e] + wa * va.v[e];
                        if (!PAD || pb >= 0) acc[u].v[e] = acc[u].v[e] + wb * vb.v[e];
                    }
                }
                if (j < k) {
                    const int64_t pa = idx_s[base + j];
                    const V va = *reinterpret_cast<const V*>(src + ((PAD && pa < 0) ? 0 : pa) * src_pitch + (int64_t)cc[u] * VEC);
                    const T wa = WEIGHTED ? w_s[base + j] : T(1);
#pragma unroll
                    for (int e = 0; e < VEC; ++e)
                        if (!PAD || pa >= 0) acc[u].v[e] = acc[u].v[e] + wa * va.v[e];
                }
            }
        }

#pragma unroll
        for (int u = 0; u < kU; ++u) {
            if (!ok[u]) continue;
            const int64_t row = tgt_rows ? (int64_t)tgt_rows[t0 + tt[u]] : t0 + tt[u];  // (uniform branch)
            if (EPI) {
                const bool masked = tgt_mask ? (tgt_mask[row] != 0) : false;
                apply_level_tables<T, VEC>(tab, n_stage, cc[u], acc[u], masked);
            }
            store_out(reinterpret_cast<V*>(out + row * out_pitch + (int64_t)cc[u] * VEC), acc[u]);
        }
    }
}

// ---------------------------------------------------------------------------------
// ATX_COLUMNS, fixed k, "direct" form: no shared memory, no barrier, no loop.  One (target, 16-byte vector) item per
// lane; a lane reads its target's k indices / weights itself (the ~35 lanes of a target read the same words: one
// request) and then the k source vectors.  Every compile-time k of the ladder below runs here, see the note at its launch
// site; the tiled kernel above serves runtime k and the epilogues that need a per-workgroup table.
// ---------------------------------------------------------------------------------
// Epilogue of the direct kernel (the fused regrid -> per-point chain, K10) without shared memory or a barrier:
//   kEpiUniform  per stage, the levels run ONE operator, or one operator up to a level and another from there on (a stack of
//                "136 levels of t, then orog" — BASELINE config 5 — or of two variables), the change falling on a 16-byte
//                vector boundary; <= kMaxUniform stages, any operators, with or without the point mask: the operators travel BY
//                VALUE in the kernel arguments (scalar registers), the dispatch on the operator is a scalar branch; with two
//                pieces both are evaluated and the lane keeps the one its vector belongs to;
//   kEpiRuns     up to 4 runs of levels per stage, boundaries anywhere (RunOps, round 4): several variables in one column, by
//                value as well; without this route such programs took the table or the tiled kernel (profiles/r04_runs_probe.log);
//   kEpiTable    programs of the multiply-add family only (COPY / AFFINE / MUL, with or without the point mask — rescale, convert,
//                orog_to_z, apply_mask: BASELINE config 5), <= kMaxTable stages, operators differing from level to level: the
//                per-VECTOR operator table the host built once (atx_vector_program, n_stage x C entries, a few hundred bytes
//                that stay in L1) is read one entry per stage and lane, REQUESTED BEFORE THE GATHER so its latency passes under
//                it, and applied without a branch (x*p0, (x*p0)+p1 and x are all formed, the operator selects: the same two
//                roundings as the statement it replaces).  Vectors whose levels differ (marker ATX_OP_MIXED) go level by level
//                through the per-level program.
// Everything else (clip / impute / exp / log / divisions, more stages) stays on the tiled kernel: its general operator switch
// costs registers (f64: 88 VGPRs, 5 waves per SIMD instead of 8) and time the gather cannot hide (profiles/r02_ab_epilogue_routes.log).
constexpr int kEpiNone = 0, kEpiUniform = 1, kEpiTable = 2, kEpiRuns = 3;
constexpr int kMaxTable = 4;

// COPY / AFFINE / MUL (+ mask) on one element, branch-free; bit-identical to apply_level_op for these operators.
template <typename T>
__device__ __forceinline__ T apply_madd_family(const LevelOp<T>& o, T x, bool masked) {
    const T m = x * o.p0;
    const T a = m + o.p1;
    T y = o.op == ATX_OP_AFFINE ? a : (o.op == ATX_OP_MUL ? m : x);
    return (o.use_mask && masked) ? quiet_nan<T>() : y;
}

template <typename T, int VEC, int K, bool WEIGHTED, bool PAD, int EPI>
__global__ void __launch_bounds__(kEllBlock)
regrid_cols_ell_direct_kernel(EllBatch batch, const int32_t* __restrict__ idx, const T* __restrict__ w, int64_t n_items,
                              int C, int64_t src_pitch, int64_t out_pitch, unsigned n_blocks, int items_per_lane,
                              UniformOps<T> uniform, const unsigned char* __restrict__ level_tables, int n_stage,
                              const uint8_t* __restrict__ tgt_mask,
                              const int32_t* __restrict__ tgt_rows, RunOps<T> runs, unsigned stripe) {
    using V = Pack<T, VEC>;
    const T* __restrict__ src = static_cast<const T*>(batch.src[blockIdx.y]);
    T* __restrict__ out = static_cast<T*>(batch.out[blockIdx.y]);
    // `stripe` (from the launcher): 0 = one contiguous range of workgroups per XCD, else stripes of that many.  (Plain round-robin
    // lost to both, profiles/r03_ell_block_sweep.log.)
    const unsigned b = stripe ? xcd_stripe(blockIdx.x, n_blocks, stripe) : xcd_tile(blockIdx.x, n_blocks);
    // items_per_lane is 1 at every launch: 2 / 4 per lane measured -4 % / -9 % (profiles/r02_items_per_lane_experiment.log).  The loop
    // form stays because the compiler allocates registers differently without it (k = 4 f32: 36 -> 26 VGPRs, every instantiation
    // moves) and this kernel's code is held to what was measured.
    for (int it = 0; it < items_per_lane; ++it) {
        const int64_t q = ((int64_t)b * items_per_lane + it) * kEllBlock + threadIdx.x;
        if (q >= n_items) return;
        const unsigned t = (unsigned)((uint64_t)q / (unsigned)C);
        const int c = (int)(q - (int64_t)t * C);
        // ordered traversal: the index / weight table is stored in the order the targets are to be visited (column blocks of the
        // target grid: vertically adjacent targets meet in L2) and row t of it belongs to output row tgt_rows[t]
        const unsigned row = tgt_rows ? (unsigned)tgt_rows[t] : t;
        int32_t p[K];
        T wv[K];
        // plain vector loads: a target's words are read again by the next wave when its vectors straddle two.  (Fetching them through the
        // scalar unit, two targets per wave and a select per lane, gained nothing: k=4 f64 0.8392 -> 0.8380 ms, k=1 f64 0.3695 -> 0.3877 —
        // the kernel waits on HBM, not on the shared words; profiles/r04_scalar_tables_experiment.log.)
#pragma unroll
        for (int j = 0; j < K; ++j) {
            p[j] = idx[(int64_t)t * K + j];
            if (WEIGHTED) wv[j] = w[(int64_t)t * K + j];
        }
        // table route: the first operators and the mask byte are requested HERE, together with the index words, so that their
        // latency passes under the gather instead of after it (loaded after the accumulation they cost 9 %: 478 vs 439 us)
        V ta[kMaxTable], tb[kMaxTable];
        unsigned tcode[kMaxTable];
        bool masked = false;
        if (EPI == kEpiUniform || EPI == kEpiRuns) masked = tgt_mask ? (tgt_mask[row] != 0) : false;
        if (EPI == kEpiTable) {  // the operators of this vector's levels, in the stack's type (level_tables_layout)
            using OpWord = typename std::conditional<VEC == 4, uint32_t, uint16_t>::type;
            const int Lp = C * VEC;
            const T* tp0 = reinterpret_cast<const T*>(level_tables);
            const T* tp1 = tp0 + (int64_t)n_stage * Lp;
            const uint8_t* tcd = reinterpret_cast<const uint8_t*>(tp1 + (int64_t)n_stage * Lp);
#pragma unroll
            for (int s = 0; s < kMaxTable; ++s) {
                tcode[s] = 0;
                if (s < n_stage) {
                    ta[s] = *reinterpret_cast<const V*>(tp0 + (int64_t)s * Lp + c * VEC);
                    tb[s] = *reinterpret_cast<const V*>(tp1 + (int64_t)s * Lp + c * VEC);
                    tcode[s] = *reinterpret_cast<const OpWord*>(tcd + (int64_t)s * Lp + c * VEC);
                }
            }
            masked = tgt_mask ? (tgt_mask[row] != 0) : false;
        }
        V v[K];
        // an absent entry of a padded row (index -1) is skipped below; its load goes to the row's FIRST column — a line this lane is
        // fetching anyway — instead of column 0, which every padded lane of the launch would share (aimed at column 0 it measured the
        // same here, profiles/r03_padded_order_probe.log; on field-major stacks the shared line cost 48 %)
        const int32_t spare = p[0] >= 0 ? p[0] : 0;
#pragma unroll
        for (int j = 0; j < K; ++j)
            v[j] = load_src<T, VEC>(src + (int64_t)((PAD && p[j] < 0) ? spare : p[j]) * src_pitch + (int64_t)c * VEC);
        V acc;
        if (WEIGHTED) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc.v[e] = T(0);
#pragma unroll
            for (int j = 0; j < K; ++j) {
                if (!PAD || p[j] >= 0) {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) acc.v[e] = acc.v[e] + wv[j] * v[j].v[e];
                }
            }
        } else {
            acc = v[0];
        }
        if (EPI == kEpiUniform) {
            for (int s = 0; s < uniform.n_stage; ++s) {
                if (uniform.split[s] >= C) {  // scalar condition: one piece
                    apply_level_op_vec<T, VEC>(uniform.stage[s], acc, masked);
                } else {
                    V other = acc;
                    apply_level_op_vec<T, VEC>(uniform.stage[s], acc, masked);
                    apply_level_op_vec<T, VEC>(uniform.second[s], other, masked);
                    if (c >= uniform.split[s]) acc = other;
                }
            }
        } else if (EPI == kEpiRuns) {
            apply_run_ops<T, VEC>(runs, c, acc, masked);
        } else if (EPI == kEpiTable) {
#pragma unroll
            for (int s = 0; s < kMaxTable; ++s) {
                if (s < n_stage) {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) {
                        const unsigned code = (tcode[s] >> (8 * e)) & 0xffu;
                        LevelOp<T> o;
                        o.op = (int)(code & 0x7fu);
                        o.use_mask = (int)(code >> 7);
                        o.p0 = ta[s].v[e];
                        o.p1 = tb[s].v[e];
                        acc.v[e] = apply_madd_family(o, acc.v[e], masked);
                    }
                }
            }
        }
        store_out(reinterpret_cast<V*>(out + (int64_t)row * out_pitch + (int64_t)c * VEC), acc);
    }
}

// ---------------------------------------------------------------------------------
// ATX_COLUMNS, general CSR.  The tile's slice of (indices, data) is contiguous in
// the CSR arrays: it is copied to LDS coalesced, then every lane walks its row
// from LDS (scipy order: sum starts at 0, entries in storage order).
// ---------------------------------------------------------------------------------
template <typename T, int VEC, bool EPI>
__global__ void __launch_bounds__(kBlock)
regrid_cols_csr_kernel(const T* __restrict__ src, T* __restrict__ out,
                       const int32_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                       const T* __restrict__ data, int64_t n_tgt, int n_lev, int C,
                       int64_t src_pitch, int64_t out_pitch, int tile, unsigned n_tiles, int cap,
                       const atx_level_op* __restrict__ prog, int n_stage,
                       const uint8_t* __restrict__ tgt_mask, const int32_t* __restrict__ tgt_rows, int stripe) {
    using V = Pack<T, VEC>;
    extern __shared__ __align__(16) unsigned char smem[];
    T* w_s = reinterpret_cast<T*>(smem);
    int32_t* idx_s = reinterpret_cast<int32_t*>(w_s + cap);
    int32_t* rp_s = idx_s + cap;
    unsigned char* prog_s = smem + (((size_t)cap * (sizeof(T) + sizeof(int32_t)) + (size_t)(tile + 1) * sizeof(int32_t) + 15) & ~size_t(15));

    const unsigned tile_id = stripe > 0 ? xcd_stripe(blockIdx.x, n_tiles, (unsigned)stripe) : xcd_tile(blockIdx.x, n_tiles);
    const int64_t t0 = (int64_t)tile_id * tile;
    const int nt = (int)min((int64_t)tile, n_tgt - t0);
    const int tid = threadIdx.x;

    for (int i = tid; i <= nt; i += kBlock) rp_s[i] = indptr[t0 + i];
    LevelTablesLds<T> tab{};  // the operators of every level (atx_common.hpp)
    if (EPI) tab = build_level_tables<T, VEC>(prog, prog_s, n_stage, n_lev, C, tid, kBlock);
    __syncthreads();
    const int64_t base = rp_s[0];
    const int nnz_tile = rp_s[nt] - rp_s[0];
    const bool staged = nnz_tile <= cap;  // block-uniform
    if (staged) {
        for (int i = tid; i < nnz_tile; i += kBlock) {
            idx_s[i] = indices[base + i];
            w_s[i] = data[base + i];
        }
    }
    __syncthreads();

    const int items = nt * C;
    for (int q = tid; q < items; q += kBlock) {
        const int t = q / C;
        const int c = q - t * C;
        const int j0 = rp_s[t] - rp_s[0], j1 = rp_s[t + 1] - rp_s[0];
        V acc;
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc.v[e] = T(0);
        int jj = j0;
        for (; jj + 4 <= j1; jj += 4) {
            int64_t p[4];
            T wv[4];
            V v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                p[u] = staged ? idx_s[jj + u] : indices[base + jj + u];
                wv[u] = staged ? w_s[jj + u] : data[base + jj + u];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const V*>(src + p[u] * src_pitch + (int64_t)c * VEC);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc.v[e] = acc.v[e] + wv[u] * v[u].v[e];
            }
        }
        for (; jj < j1; ++jj) {
            const int64_t p = staged ? idx_s[jj] : indices[base + jj];
            const T wv = staged ? w_s[jj] : data[base + jj];
            const V v = *reinterpret_cast<const V*>(src + p * src_pitch + (int64_t)c * VEC);
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc.v[e] = acc.v[e] + wv * v.v[e];
        }
        const int64_t row = tgt_rows ? (int64_t)tgt_rows[t0 + t] : t0 + t;  // ordered traversal: CSR row t is output row tgt_rows[t]
        if (EPI) {
            const bool masked = tgt_mask ? (tgt_mask[row] != 0) : false;
            apply_level_tables<T, VEC>(tab, n_stage, c, acc, masked);
        }
        store_out(reinterpret_cast<V*>(out + row * out_pitch + (int64_t)c * VEC), acc);
    }
}

// ---------------------------------------------------------------------------------
// host-side launchers
// ---------------------------------------------------------------------------------

// Every operator of the program is COPY, AFFINE or MUL (masked or not) and there are <= kMaxTable stages: the direct
// kernel's table route applies.
static bool madd_family_program(const Epilogue& e, int n_lev) {
    if (!e.host_prog || !e.vec_prog || !aligned16(e.vec_prog) || e.n_stage < 1 || e.n_stage > kMaxTable) return false;
    for (int64_t i = 0; i < (int64_t)e.n_stage * n_lev; ++i) {
        const int op = e.host_prog[i].op;
        if (op != ATX_OP_COPY && op != ATX_OP_AFFINE && op != ATX_OP_MUL) return false;
    }
    return true;
}

// Per stage the levels run one operator, or one up to a level that is a multiple of `vec` and another from there on
// (<= kMaxUniform stages): the operators can travel by value (atx_common.hpp: uniform_level_program).
template <typename T>
static bool uniform_program(const Epilogue& e, int n_lev, int vec, UniformOps<T>& out) {
    return uniform_level_program<T>(e.host_prog, e.n_stage, e.mask != nullptr, n_lev, vec, out);
}

template <typename T, int VEC, int K, bool WEIGHTED, bool PAD = false>
static int launch_cols_ell(const EllBatch& batch, const int32_t* idx, const T* w, int64_t n_tgt, int k,
                           int n_lev, int64_t src_pitch, int64_t out_pitch, const Epilogue& epi, hipStream_t stream) {
    const int C = (n_lev + VEC - 1) / VEC;
    const atx_level_op* prog = epi.prog;
    const int n_stage = epi.n_stage;
    const uint8_t* tgt_mask = epi.mask;
    // Fixed-k gathers with compile-time k (1-8, 12, 16; padded ragged rows from 3) take the direct kernel.  Interleaved A/B on O1280 ->
    // 0.25 deg, 137 levels (profiles/r01_ab_direct_kernel.log): k=4 f32 0.4360 vs 0.4378 ms, k=1 f32 0.1926 vs 0.1992 ms, k=4 f64 0.8334 vs
    // 0.8343 ms; 1-60 levels equal or up to 15 % faster; 2 / 4 items per lane -4 % / -9 %.  Same bits, no tile heuristic to tune.
    // With an epilogue it still does when the operators can reach it without a per-workgroup set-up: by value (uniform
    // program seen through host_prog) or, for multiply-add programs, through the host-built per-vector table (vec_prog);
    // profiles/r02_ab_epilogue_routes.log.  Round 3 tried TWO vectors per lane (columns c and c + ceil(C/2) of one target: half the
    // lanes read the index / weight words, 2 k source loads in flight per lane) — slower everywhere: k=4 f64 0.841 -> 0.912 ms,
    // k=1 f64 0.368 -> 0.420, k=4 f32 0.439 -> 0.523, k=1 f32 0.197 -> 0.236 (profiles/r03_direct_v2_experiment.log); one item per
    // lane in many short waves it stays.
    if constexpr (K > 0) {
        if (g_tile_override <= 0) {  // atx_set_tuning(tile > 0) selects the tiled kernel below (A/B, tests)
            const int64_t n_items = n_tgt * C;
            const unsigned n_blocks = (unsigned)((n_items + kEllBlock - 1) / kEllBlock);
            // Long rows in the caller's own (natural) order: deal the workgroups to the XCDs in stripes of 64 instead of one contiguous range
            // each.  The cost of a long row varies with latitude (polar targets share their source columns, equatorial ones fetch every one
            // from HBM) and a contiguous range keeps an XCD on one belt for the whole launch: O1280 -> 0.25 degree, k = 16 0.52 -> 0.59 (f32) /
            // 0.56 (f64) of the HBM peak, k = 8 +2-6 %; rows of up to 4 entries gain nothing (-0.5 .. -4 %), and an ORDERED launch (tgt_rows:
            // full-height column blocks, which balance by themselves) loses 5-8 % to stripes (profiles/r04_xcd_stripes_experiment.log).
            const unsigned stripe = (K >= 5 && !epi.tgt_rows) ? kLongRowStripe : 0u;
            UniformOps<T> uniform{};
            RunOps<T> runs{};
            const unsigned char* level_tables = nullptr;
            auto direct = [&](auto kind, const char* what, const char* epilogue) {
                g_gather_route = GatherRoute{"cols_ell", "direct", epilogue, VEC == 1 ? "scalar" : "vec", K, PAD, WEIGHTED, stripe != 0, epi.tgt_rows != nullptr, false};
                hipLaunchKernelGGL((regrid_cols_ell_direct_kernel<T, VEC, K, WEIGHTED, PAD, decltype(kind)::value>), dim3(n_blocks, batch.n),
                                   dim3(kEllBlock), 0, stream, batch, idx, w, n_items, C, src_pitch, out_pitch, n_blocks, 1, uniform, level_tables,
                                   n_stage, tgt_mask, epi.tgt_rows, runs, stripe);
                ATX_LAUNCH_CHECK(what);
                return (int)ATX_OK;
            };
            if (!prog) return direct(IntTag<kEpiNone>{}, "regrid_cols_ell_direct", "none");
            if (uniform_program<T>(epi, n_lev, VEC, uniform)) return direct(IntTag<kEpiUniform>{}, "regrid_cols_ell_direct_uniform", "uniform");
            // several variables in one column (runs of levels with boundaries anywhere): by value, no table read beside the gather
            if (runs_level_program<T>(epi.host_prog, n_stage, tgt_mask != nullptr, n_lev, runs)) return direct(IntTag<kEpiRuns>{}, "regrid_cols_ell_direct_runs", "runs");
            if (VEC == Vec16<T>::N && madd_family_program(epi, n_lev)) {  // the table is built for 16-byte vectors
                level_tables = reinterpret_cast<const unsigned char*>(epi.vec_prog) +
                               level_tables_layout(n_stage, n_lev, sizeof(T) == 4 ? ATX_F32 : ATX_F64).levels_offset;
                return direct(IntTag<kEpiTable>{}, "regrid_cols_ell_direct_table", "table");
            }
        }
    }
    int tile = g_tile_override > 0 ? g_tile_override : pick_tile(n_tgt, C, prog != nullptr);
    if ((int64_t)tile > n_tgt) tile = (int)n_tgt;
    // the tile's index / weight rows live in LDS: long rows on a THIN stack (pick_tile sizes tiles by items, so few levels mean many
    // targets: k = 64 over 4 levels asked for 196 KB) get as many targets as fit in 48 KB, whatever the tuning hook says
    const size_t row_bytes = (size_t)k * (sizeof(int32_t) + (WEIGHTED ? sizeof(T) : 0));
    if ((size_t)tile * row_bytes > 48 * 1024) tile = (int)(48 * 1024 / row_bytes) > 4 ? (int)(48 * 1024 / row_bytes) / 4 * 4 : 1;
    const unsigned n_tiles = (unsigned)((n_tgt + tile - 1) / tile);
    size_t lds = (size_t)tile * row_bytes;
    lds = (lds + 15) & ~size_t(15);
    if (prog) lds += level_tables_lds_bytes<T>(n_stage, C, VEC);
    if (prog && lds > 64 * 1024) return ATX_SPLIT_PROGRAM;  // the caller gathers without the program and applies it afterwards
    ATX_REQUIRE(lds <= 64 * 1024, ATX_ENOTIMPL, "regrid_ell: tile needs %zu B of LDS (k=%d, n_lev=%d, stages=%d)", lds, k, n_lev, n_stage);
    constexpr int KT = K > 4 ? 0 : K;  // the tiled kernel keeps k > 4 on its runtime-k loop (compile-time k would hold 4 x k vectors per lane)
    g_gather_route = GatherRoute{"cols_ell", "tiled", prog ? "lds" : "none", VEC == 1 ? "scalar" : "vec", KT, PAD, WEIGHTED, false, epi.tgt_rows != nullptr, false};
    with_flag(prog != nullptr, [&](auto fused) {
        hipLaunchKernelGGL((regrid_cols_ell_kernel<T, VEC, KT, WEIGHTED, decltype(fused)::value, PAD>), dim3(n_tiles, batch.n), dim3(kEllBlock), lds, stream,
                           batch, idx, w, n_tgt, k, n_lev, C, src_pitch, out_pitch, tile, n_tiles, prog, n_stage, tgt_mask, epi.tgt_rows);
    });
    ATX_LAUNCH_CHECK("regrid_cols_ell");
    return ATX_OK;
}

template <typename T, int VEC>
static int dispatch_cols_ell(const EllBatch& batch, const int32_t* idx, const T* w, int64_t n_tgt, int k,
                             int n_lev, int64_t sp, int64_t op, bool pad, const Epilogue& e, hipStream_t st) {
    if (!w) return launch_cols_ell<T, VEC, 1, false>(batch, idx, w, n_tgt, k, n_lev, sp, op, e, st);
    return with_flag(pad, [&](auto padded) {
        constexpr bool PAD = decltype(padded)::value;
        constexpr int kMin = PAD ? 3 : 1;  // padded ragged rows: compile-time k from 3 (shorter padded tables take the runtime-k loop)
        auto fixed = [&](auto kc) {
            constexpr int K = decltype(kc)::value >= kMin ? decltype(kc)::value : 0;
            return launch_cols_ell<T, VEC, K, true, PAD>(batch, idx, w, n_tgt, k, n_lev, sp, op, e, st);
        };
        switch (k) {
            case 1: return fixed(IntTag<1>{});
            case 2: return fixed(IntTag<2>{});
            case 3: return fixed(IntTag<3>{});
            case 4: return fixed(IntTag<4>{});
            // compile-time k up to 8 (the direct kernel: all k loads of an item in flight at once); k = 5 .. 8 moved off the runtime-k tiled
            // kernel in round 3: k = 8 0.608 -> 0.635 f32, 0.625 -> 0.657 f64, k = 6 0.636 -> 0.650 / 0.659 -> 0.683 (profiles/r03_mid_k_experiment.log)
            case 5: return fixed(IntTag<5>{});
            case 6: return fixed(IntTag<6>{});
            case 7: return fixed(IntTag<7>{});
            case 8: return fixed(IntTag<8>{});
            // the two round numbers beyond 8 a k-NN regrid is configured with: all 12 / 16 source vectors in flight beat the tiled kernel's
            // runtime-k loop (k = 16: 0.46 -> 0.51 f32 in natural order, 0.58 with the targets in column blocks, f64 0.48 -> 0.52 / 0.54);
            // a runtime-k loop IN the direct kernel, 8 or 16 entries per step, measured no better than the tiled kernel and was dropped
            // (profiles/r03_long_k_direct_experiment.log)
            case 12: return fixed(IntTag<12>{});
            case 16: return fixed(IntTag<16>{});
            default: return fixed(IntTag<0>{});
        }
    });
}

template <typename T, int VEC>
static int launch_cols_csr(const T* src, T* out, const int32_t* indptr, const int32_t* indices, const T* data,
                           int64_t n_tgt, int64_t nnz, int n_lev, int64_t sp, int64_t op,
                           const atx_level_op* prog, int n_stage, const uint8_t* m, const int32_t* rows, hipStream_t st) {
    const int C = (n_lev + VEC - 1) / VEC;
    // (A "direct" form of this kernel — one item per lane, row walked from the CSR arrays in L1 — was measured and dropped: rows of
    // 3-4 entries 0.478 ms against 0.450 ms tiled, rows of 9-16 entries 1.06 against 1.01 ms f32, 2.03 against 2.10 ms f64; with 8
    // entries in flight and the next step's words prefetched 1.10 ms.  The extra dependent load level — row bounds, entries, source
    // columns — costs what the missing barrier saves; profiles/r02_csr_direct_experiment.log.  Nor do long rows want more loads in
    // flight: box-average coarsening O1280 -> 1 degree, ~100 entries per row, every source column read exactly once, runs at 0.86 ms
    // = 4.3 TB/s with 4 entries per step and 0.85 ms with 8 (at 84 VGPRs, 5 waves per SIMD), whatever the tile size —
    // profiles/r02_long_rows_experiment.log.)
    int tile = g_tile_override > 0 ? g_tile_override : pick_tile(n_tgt, C, prog != nullptr);
    if ((int64_t)tile > n_tgt) tile = (int)n_tgt;
    const unsigned n_tiles = (unsigned)((n_tgt + tile - 1) / tile);
    // LDS room for ~2x the mean entries of a tile (tiles above it read CSR from L2)
    const double mean = n_tgt > 0 ? (double)nnz / (double)n_tgt : 0.0;
    int cap = (int)(mean * tile * 2.0) + 64;
    if (cap > 4096) cap = 4096;
    size_t lds = (size_t)cap * (sizeof(T) + sizeof(int32_t)) + (size_t)(tile + 1) * sizeof(int32_t);
    lds = (lds + 15) & ~size_t(15);
    if (prog) lds += level_tables_lds_bytes<T>(n_stage, C, VEC);
    if (prog && lds > 64 * 1024) return ATX_SPLIT_PROGRAM;  // the caller gathers without the program and applies it afterwards
    ATX_REQUIRE(lds <= 64 * 1024, ATX_ENOTIMPL, "regrid_csr: tile needs %zu B of LDS", lds);
    // long rows in natural order: stripes of tiles per XCD (atx_common.hpp: xcd_stripe) — their cost may drift along the rows.  Box
    // averages with rows of ~25: 0.859 -> 0.692 ms f32, 1.901 -> 1.363 ms f64; rows of 3-4 lose 2 % to stripes; 4 and 64 tiles per
    // stripe no better than 16 (profiles/r03_csr_stripes.log, tools/experiments/csr_stripes.py)
    const int stripe = (!rows && mean >= kCsrStripeMinMean) ? kCsrStripe : 0;
    g_gather_route = GatherRoute{"cols_csr", "tiled", prog ? "lds" : "none", VEC == 1 ? "scalar" : "vec", 0, false, true, stripe != 0, rows != nullptr, false};
    with_flag(prog != nullptr, [&](auto fused) {
        hipLaunchKernelGGL((regrid_cols_csr_kernel<T, VEC, decltype(fused)::value>), dim3(n_tiles), dim3(kBlock), lds, st, src, out, indptr,
                           indices, data, n_tgt, n_lev, C, sp, op, tile, n_tiles, cap, prog, n_stage, m, rows, stripe);
    });
    ATX_LAUNCH_CHECK("regrid_cols_csr");
    return ATX_OK;
}

// A column stack of one element type: the vector path needs every row start 16-byte aligned and room for the last (partial) vector
// inside the pitch; anything else takes the scalar (VEC = 1) instantiations.
template <typename T>
static int regrid_cols_ell(const EllBatch& batch, const int32_t* idx, const T* w, int64_t n_tgt, int k, int n_lev, int64_t sp, int64_t op,
                           bool pad, const Epilogue& e, hipStream_t st) {
    constexpr int VEC = Vec16<T>::N;
    const int64_t covered = ((int64_t)(n_lev + VEC - 1) / VEC) * VEC;
    bool vector_ok = covered <= sp && covered <= op;
    for (int i = 0; i < batch.n; ++i) vector_ok = vector_ok && cols_vector_ok<T>(batch.src[i], batch.out[i], sp, op);
    if (vector_ok) return dispatch_cols_ell<T, VEC>(batch, idx, w, n_tgt, k, n_lev, sp, op, pad, e, st);
    return dispatch_cols_ell<T, 1>(batch, idx, w, n_tgt, k, n_lev, sp, op, pad, e, st);
}

template <typename T>
static int regrid_cols_csr(const T* src, T* out, const int32_t* indptr, const int32_t* indices, const T* data, int64_t n_tgt, int64_t nnz,
                           int n_lev, int64_t sp, int64_t op, const atx_level_op* prog, int n_stage, const uint8_t* m, const int32_t* rows,
                           hipStream_t st) {
    constexpr int VEC = Vec16<T>::N;
    const int64_t covered = ((int64_t)(n_lev + VEC - 1) / VEC) * VEC;
    if (cols_vector_ok<T>(src, out, sp, op) && covered <= sp && covered <= op)
        return launch_cols_csr<T, VEC>(src, out, indptr, indices, data, n_tgt, nnz, n_lev, sp, op, prog, n_stage, m, rows, st);
    return launch_cols_csr<T, 1>(src, out, indptr, indices, data, n_tgt, nnz, n_lev, sp, op, prog, n_stage, m, rows, st);
}

}  // namespace atx
