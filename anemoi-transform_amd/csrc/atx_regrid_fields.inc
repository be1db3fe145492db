// The gather on ATX_FIELDS stacks (the reference's array order; DESIGN.md §3): lane = target, the row's neighbour indices / weights
// live in registers and are reused for every level of the level chunk (grid.y).
//  * regrid_fields_ell_kernel       fixed k: compile-time 1..4 (padded ragged rows 3, 4), else a runtime-k loop over 16 fields;
//  * regrid_fields_csr_head_kernel  general CSR, short rows (mean <= 8 entries): the first R entries in registers;
//  * regrid_fields_csr_kernel       general CSR, longer rows: the row walked once per chunk of kFieldsChunk fields.
// A row of more than ~8 entries re-fetches every source point once per row that uses it: GatherPlan.apply converts such stacks to
// columns first.  Included by atx_regrid_typed.inc; the helpers shared with the columns piece are in atx_regrid_decl.hpp.

namespace atx {

// ---------------------------------------------------------------------------------
// ATX_FIELDS, fixed k.  lane = target; grid.y = level chunk.
// ---------------------------------------------------------------------------------
template <typename T, int K, bool WEIGHTED, bool EPI, bool PAD>
__global__ void __launch_bounds__(kBlock)
regrid_fields_ell_kernel(const T* __restrict__ src, T* __restrict__ out,
                         const int32_t* __restrict__ idx, const T* __restrict__ w,
                         int64_t n_tgt, int k_rt, int n_lev, int64_t src_pitch, int64_t out_pitch,
                         int lev_chunk, unsigned n_tiles,
                         const atx_level_op* __restrict__ prog, int n_stage,
                         const uint8_t* __restrict__ tgt_mask) {
    const int k = K > 0 ? K : k_rt;
    const unsigned tile_id = xcd_tile(blockIdx.x, n_tiles);
    const int64_t t = (int64_t)tile_id * kBlock + threadIdx.x;
    if (t >= n_tgt) return;
    const int l0 = blockIdx.y * lev_chunk;
    const int l1 = min(n_lev, l0 + lev_chunk);
    const bool masked = (EPI && tgt_mask) ? (tgt_mask[t] != 0) : false;

    if (K > 0) {
        int64_t p[K > 0 ? K : 1];
        T wj[K > 0 ? K : 1];
        bool present[K > 0 ? K : 1];
#pragma unroll
        for (int j = 0; j < (K > 0 ? K : 1); ++j) {
            p[j] = idx[t * K + j];
            wj[j] = WEIGHTED ? w[t * K + j] : T(1);
            present[j] = !PAD || p[j] >= 0;  // absent entry of a padded row
        }
        if (PAD) {  // an absent entry reads what the row's first entry reads (a line this lane fetches anyway), not element 0 of every field —
            // that one line, shared by every padded lane of the launch, cost 48 % (ragged 3-4 rows padded to 4: 1.12 ms against 0.76 ms)
            const int64_t spare = present[0] ? p[0] : 0;
#pragma unroll
            for (int j = 0; j < (K > 0 ? K : 1); ++j)
                if (!present[j]) p[j] = spare;
        }
#pragma unroll 4
        for (int l = l0; l < l1; ++l) {
            const T* s = src + (int64_t)l * src_pitch;
            T acc;
            if (WEIGHTED) {
                // all k loads first, unconditionally; the sum then skips absent entries by a select.  (Written as `if (present[j])
                // acc += w * s[p]` the padded instantiation put each load behind a divergent branch: the SAME k = 4 table ran in
                // 1.03 ms through it against 0.70 ms through the plain one.)
                T sv[K > 0 ? K : 1];
#pragma unroll
                for (int j = 0; j < (K > 0 ? K : 1); ++j) sv[j] = s[p[j]];
                acc = T(0);
#pragma unroll
                for (int j = 0; j < (K > 0 ? K : 1); ++j) {
                    const T sum = acc + wj[j] * sv[j];
                    acc = present[j] ? sum : acc;
                }
            } else {
                acc = s[p[0]];
            }
            if (EPI) {
                for (int st = 0; st < n_stage; ++st)
                    acc = apply_level_op(load_level_op<T>(prog, (int64_t)st * n_lev + l), acc, masked);
            }
            store_field(out + (int64_t)l * out_pitch + t, acc);  // written through (atx_regrid_decl.hpp)
        }
    } else {  // run-time k: the row walked once per 16 fields, one accumulator per field (cf. regrid_fields_csr_kernel)
        constexpr int LC = 16;
        for (int lc = l0; lc < l1; lc += LC) {
            const int nl = min(LC, l1 - lc);  // (uniform)
            const T* s0 = src + (int64_t)lc * src_pitch;
            T acc[LC];
#pragma unroll
            for (int i = 0; i < LC; ++i) acc[i] = T(0);
            for (int j = 0; j < k; ++j) {
                const T wv = WEIGHTED ? w[t * k + j] : T(1);
                const int64_t pj = idx[t * k + j];
                if (PAD && pj < 0) continue;
#pragma unroll
                for (int i = 0; i < LC; ++i)
                    if (i < nl) acc[i] = acc[i] + wv * s0[(int64_t)i * src_pitch + pj];
            }
#pragma unroll
            for (int i = 0; i < LC; ++i) {
                if (i < nl) {
                    T v = acc[i];
                    if (EPI) {
                        for (int st = 0; st < n_stage; ++st)
                            v = apply_level_op(load_level_op<T>(prog, (int64_t)st * n_lev + lc + i), v, masked);
                    }
                    out[(int64_t)(lc + i) * out_pitch + t] = v;  // plain store: store_field was measured on the compile-time k route only
                }
            }
        }
    }
}

// ATX_FIELDS, general CSR: lane = row, grid.y = chunk of kFieldsChunk fields.  The row is walked ONCE per chunk — entry by entry, the
// entry's index and weight in registers while its kFieldsChunk gathers (one per field, all independent) are in flight — with one
// accumulator per field of the chunk; every field still sums its row in storage order starting from 0 (scipy's order).  Until round 3
// the loops were nested the other way, each field re-reading every index and weight and chaining its gathers: O1280 -> 0.25 deg,
// 137 fields, ragged rows of 3-4 entries 1.97 ms (the fixed-k kernel: 0.76 ms), rows of 9-16 entries 17 ms (float32).
// Short rows (mean <= R entries): the first R entries of the row in registers for all fields of the chunk (absent ones point at the
// row's first entry and are skipped by a select), entries beyond R re-read per field.  Ragged rows of 3-4 entries: 1.97 -> 1.11 ms.
template <typename T, bool EPI, int R>
__global__ void __launch_bounds__(kBlock)
regrid_fields_csr_head_kernel(const T* __restrict__ src, T* __restrict__ out,
                              const int32_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                              const T* __restrict__ data, int64_t n_tgt, int n_lev,
                              int64_t src_pitch, int64_t out_pitch, int lev_chunk, unsigned n_tiles,
                              const atx_level_op* __restrict__ prog, int n_stage,
                              const uint8_t* __restrict__ tgt_mask) {
    const unsigned tile_id = xcd_tile(blockIdx.x, n_tiles);
    const int64_t t = (int64_t)tile_id * kBlock + threadIdx.x;
    if (t >= n_tgt) return;
    const int l0 = blockIdx.y * lev_chunk;
    const int l1 = min(n_lev, l0 + lev_chunk);
    const int64_t j0 = indptr[t], j1 = indptr[t + 1];
    const bool masked = (EPI && tgt_mask) ? (tgt_mask[t] != 0) : false;
    int64_t p[R];
    T wj[R];
    bool present[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
        present[j] = j0 + j < j1;
        p[j] = present[j] ? (int64_t)indices[j0 + j] : (j > 0 ? p[0] : 0);
        wj[j] = present[j] ? data[j0 + j] : T(0);
    }
    const int64_t rest = j0 + R;
#pragma unroll 4
    for (int l = l0; l < l1; ++l) {
        const T* s = src + (int64_t)l * src_pitch;
        T sv[R];
#pragma unroll
        for (int j = 0; j < R; ++j) sv[j] = s[p[j]];
        T acc = T(0);
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const T sum = acc + wj[j] * sv[j];
            acc = present[j] ? sum : acc;
        }
        for (int64_t jj = rest; jj < j1; ++jj) acc = acc + data[jj] * s[indices[jj]];
        if (EPI) {
            for (int st = 0; st < n_stage; ++st)
                acc = apply_level_op(load_level_op<T>(prog, (int64_t)st * n_lev + l), acc, masked);
        }
        out[(int64_t)l * out_pitch + t] = acc;
    }
}

constexpr int kFieldsChunk = 16;
template <typename T, bool EPI>
__global__ void __launch_bounds__(kBlock)
regrid_fields_csr_kernel(const T* __restrict__ src, T* __restrict__ out,
                         const int32_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                         const T* __restrict__ data, int64_t n_tgt, int n_lev,
                         int64_t src_pitch, int64_t out_pitch, unsigned n_tiles,
                         const atx_level_op* __restrict__ prog, int n_stage,
                         const uint8_t* __restrict__ tgt_mask) {
    const unsigned tile_id = xcd_tile(blockIdx.x, n_tiles);
    const int64_t t = (int64_t)tile_id * kBlock + threadIdx.x;
    if (t >= n_tgt) return;
    const int l0 = blockIdx.y * kFieldsChunk;
    const int nl = min(kFieldsChunk, n_lev - l0);  // (uniform)
    const int64_t j0 = indptr[t], j1 = indptr[t + 1];
    const T* s0 = src + (int64_t)l0 * src_pitch;
    T acc[kFieldsChunk];
#pragma unroll
    for (int i = 0; i < kFieldsChunk; ++i) acc[i] = T(0);
    for (int64_t jj = j0; jj < j1; ++jj) {
        const int64_t p = indices[jj];
        const T wv = data[jj];
#pragma unroll
        for (int i = 0; i < kFieldsChunk; ++i)
            if (i < nl) acc[i] = acc[i] + wv * s0[(int64_t)i * src_pitch + p];
    }
    const bool masked = (EPI && tgt_mask) ? (tgt_mask[t] != 0) : false;
#pragma unroll
    for (int i = 0; i < kFieldsChunk; ++i) {
        if (i < nl) {
            T v = acc[i];
            if (EPI) {
                for (int st = 0; st < n_stage; ++st)
                    v = apply_level_op(load_level_op<T>(prog, (int64_t)st * n_lev + l0 + i), v, masked);
            }
            out[(int64_t)(l0 + i) * out_pitch + t] = v;
        }
    }
}

// ---------------------------------------------------------------------------------
// host-side launchers
// ---------------------------------------------------------------------------------
template <typename T, int K, bool WEIGHTED, bool PAD = false>
static int launch_fields_ell(const T* src, T* out, const int32_t* idx, const T* w, int64_t n_tgt, int k,
                             int n_lev, int64_t sp, int64_t op, const atx_level_op* prog, int n_stage,
                             const uint8_t* m, hipStream_t st) {
    const unsigned n_tiles = (unsigned)((n_tgt + kBlock - 1) / kBlock);
    const int lev_chunk = pick_lev_chunk(n_lev);
    const unsigned n_chunks = (unsigned)((n_lev + lev_chunk - 1) / lev_chunk);
    ATX_REQUIRE(n_chunks <= 65535, ATX_ENOTIMPL, "regrid_ell: too many level chunks (%u)", n_chunks);
    g_gather_route = GatherRoute{"fields_ell", "lanes", prog ? "global" : "none", "lane", K, PAD, WEIGHTED, false, false, false};
    with_flag(prog != nullptr, [&](auto fused) {
        hipLaunchKernelGGL((regrid_fields_ell_kernel<T, K, WEIGHTED, decltype(fused)::value, PAD>), dim3(n_tiles, n_chunks), dim3(kBlock), 0, st,
                           src, out, idx, w, n_tgt, k, n_lev, sp, op, lev_chunk, n_tiles, prog, n_stage, m);
    });
    ATX_LAUNCH_CHECK("regrid_fields_ell");
    return ATX_OK;
}

template <typename T>
static int dispatch_fields_ell(const T* src, T* out, const int32_t* idx, const T* w, int64_t n_tgt, int k,
                               int n_lev, int64_t sp, int64_t op, bool pad, const atx_level_op* prog, int n_stage,
                               const uint8_t* m, hipStream_t st) {
    if (!w) return launch_fields_ell<T, 1, false>(src, out, idx, w, n_tgt, k, n_lev, sp, op, prog, n_stage, m, st);
    return with_flag(pad, [&](auto padded) {
        constexpr bool PAD = decltype(padded)::value;
        constexpr int kMin = PAD ? 3 : 1;  // padded ragged rows: compile-time k from 3, as on column stacks
        auto fixed = [&](auto kc) {
            constexpr int K = decltype(kc)::value >= kMin ? decltype(kc)::value : 0;
            return launch_fields_ell<T, K, true, PAD>(src, out, idx, w, n_tgt, k, n_lev, sp, op, prog, n_stage, m, st);
        };
        switch (k) {
            case 1: return fixed(IntTag<1>{});
            case 2: return fixed(IntTag<2>{});
            case 3: return fixed(IntTag<3>{});
            case 4: return fixed(IntTag<4>{});
            default: return fixed(IntTag<0>{});
        }
    });
}

// Field-major stacks: lanes keep indices / weights in registers, one launch per stack of the batch.
template <typename T>
static int regrid_fields_ell(const EllBatch& batch, const int32_t* idx, const T* w, int64_t n_tgt, int k, int n_lev, int64_t sp, int64_t op,
                             bool pad, const Epilogue& e, hipStream_t st) {
    for (int i = 0; i < batch.n; ++i) {
        const int rc = dispatch_fields_ell<T>(static_cast<const T*>(batch.src[i]), static_cast<T*>(batch.out[i]), idx, w, n_tgt, k,
                                              n_lev, sp, op, pad, e.prog, e.n_stage, e.mask, st);
        if (rc != ATX_OK) return rc;
    }
    return ATX_OK;
}

template <typename T>
static int regrid_fields_csr(const T* src, T* out, const int32_t* indptr, const int32_t* indices, const T* data, int64_t n_tgt, int64_t nnz,
                             int n_lev, int64_t sp, int64_t op, const atx_level_op* prog, int n_stage, const uint8_t* m, const int32_t* rows,
                             hipStream_t st) {
    ATX_REQUIRE(!rows, ATX_ENOTIMPL, "regrid_csr: an ordered traversal (tgt_rows) is available for ATX_COLUMNS stacks only");
    const unsigned n_tiles = (unsigned)((n_tgt + kBlock - 1) / kBlock);
    const double mean = n_tgt > 0 ? (double)nnz / (double)n_tgt : 0.0;
    if (mean <= 8.0) {  // short rows: their entries in registers
        const int lev_chunk = pick_lev_chunk(n_lev);
        const unsigned chunks = (unsigned)((n_lev + lev_chunk - 1) / lev_chunk);
        ATX_REQUIRE(chunks <= 65535, ATX_ENOTIMPL, "regrid_csr: too many level chunks (%u)", chunks);
        g_gather_route = GatherRoute{"fields_csr", mean <= 4.0 ? "head4" : "head8", prog ? "global" : "none", "lane", 0, false, true, false, false, false};
        with_flag(prog != nullptr, [&](auto fused) {
            with_flag(mean <= 4.0, [&](auto four) {
                hipLaunchKernelGGL((regrid_fields_csr_head_kernel<T, decltype(fused)::value, decltype(four)::value ? 4 : 8>), dim3(n_tiles, chunks),
                                   dim3(kBlock), 0, st, src, out, indptr, indices, data, n_tgt, n_lev, sp, op, lev_chunk, n_tiles, prog, n_stage, m);
            });
        });
        ATX_LAUNCH_CHECK("regrid_fields_csr_head");
        return ATX_OK;
    }
    const unsigned n_chunks = (unsigned)((n_lev + kFieldsChunk - 1) / kFieldsChunk);
    ATX_REQUIRE(n_chunks <= 65535, ATX_ENOTIMPL, "regrid_csr: too many level chunks (%u)", n_chunks);
    g_gather_route = GatherRoute{"fields_csr", "long", prog ? "global" : "none", "lane", 0, false, true, false, false, false};
    with_flag(prog != nullptr, [&](auto fused) {
        hipLaunchKernelGGL((regrid_fields_csr_kernel<T, decltype(fused)::value>), dim3(n_tiles, n_chunks), dim3(kBlock), 0, st, src, out, indptr, indices,
                           data, n_tgt, n_lev, sp, op, n_tiles, prog, n_stage, m);
    });
    ATX_LAUNCH_CHECK("regrid_fields_csr");
    return ATX_OK;
}

}  // namespace atx
