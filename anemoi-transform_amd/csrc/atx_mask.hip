// Point masks: the predicate that builds one, its population count, and the stable compaction mask -> ascending index list.
//
// Replaces the boolean arrays and boolean indexing of the reference
//   R: filters/fields/apply_mask.py:160-163   OPERATORS[op](mask_values, threshold) / mask_values == mask_value
//   R: filters/fields/remove_nans.py:101      ~np.isnan(data)
//   R: filters/fields/remove_nans.py:110-116, regrid.py:420   data[bool_mask] (through the index list and a k = 1 gather)
// by uint8 masks that stay on the device.  atx_mask_build is HBM-bound (one pass over the field, one byte out per point); the
// count and the compaction read one byte per point and are launch-bound on one field: two launches up to kCompactSelfScan
// workgroups, three beyond.
#include "atx_common.hpp"

namespace atx {

template <typename T>
__device__ __forceinline__ bool compare(T m, T thr, int cmp) {
    switch (cmp) {
        case ATX_CMP_GT: return m > thr;
        case ATX_CMP_LT: return m < thr;
        case ATX_CMP_EQ: return m == thr;
        case ATX_CMP_NE: return m != thr;  // true for NaN, like np.not_equal
        case ATX_CMP_GE: return m >= thr;
        case ATX_CMP_LE: return m <= thr;
        case ATX_CMP_NOTNAN: return m == m;
        case ATX_CMP_ISNAN: return m != m;
        default: return false;
    }
}

template <typename T>
__global__ void __launch_bounds__(kBlock)
mask_build_kernel(const T* __restrict__ m, int64_t m_stride, uint8_t* __restrict__ mask, int64_t n, int cmp, T thr) {
    // 4 points per lane -> one 32-bit store of 4 mask bytes
    const int64_t n4 = n / 4;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kBlock) {
        uint32_t packed = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) packed |= (compare<T>(m[(i * 4 + e) * m_stride], thr, cmp) ? 1u : 0u) << (8 * e);
        *reinterpret_cast<uint32_t*>(mask + i * 4) = packed;
    }
    if (blockIdx.x == 0 && threadIdx.x < 4) {
        const int64_t i = n4 * 4 + threadIdx.x;
        if (i < n) mask[i] = compare<T>(m[i * m_stride], thr, cmp) ? 1 : 0;
    }
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    return v;
}

__global__ void __launch_bounds__(kBlock)
mask_count_kernel(const uint8_t* __restrict__ mask, int64_t n, unsigned long long* count) {
    unsigned long long c = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
        c += mask[i] != 0;
    c = wave_sum(c);
    if ((threadIdx.x & (kWave - 1)) == 0 && c) atomicAdd(count, c);
}

// ---- stable compaction: mask -> ascending index list ------------------------------
constexpr int kPerLane = 16;                     // mask bytes per lane
constexpr int kChunk = kBlock * kPerLane;        // mask bytes per workgroup

__device__ __forceinline__ int lane_count(const uint8_t* __restrict__ mask, int64_t base, int64_t n, uint32_t& bits) {
    bits = 0;
#pragma unroll
    for (int e = 0; e < kPerLane; ++e) {
        const int64_t i = base + e;
        if (i < n && mask[i] != 0) bits |= 1u << e;
    }
    return __popc(bits);
}

__global__ void __launch_bounds__(kBlock)
compact_count_kernel(const uint8_t* __restrict__ mask, int64_t n, int32_t* __restrict__ block_counts) {
    __shared__ unsigned long long wsum[kBlock / kWave];
    uint32_t bits;
    const int64_t base = (int64_t)blockIdx.x * kChunk + (int64_t)threadIdx.x * kPerLane;
    unsigned long long c = wave_sum((unsigned long long)lane_count(mask, base, n, bits));
    if ((threadIdx.x & (kWave - 1)) == 0) wsum[threadIdx.x / kWave] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int i = 0; i < kBlock / kWave; ++i) t += wsum[i];
        block_counts[blockIdx.x] = (int32_t)t;
    }
}

// single workgroup: exclusive scan of the per-block counts, in place
__global__ void __launch_bounds__(1024)
compact_scan_kernel(int32_t* __restrict__ block_counts, int n_blocks, long long* __restrict__ total) {
    __shared__ long long part[1024];
    const int tid = threadIdx.x;
    const int per = (n_blocks + 1023) / 1024;
    const int b0 = tid * per, b1 = min(n_blocks, b0 + per);
    long long s = 0;
    for (int b = b0; b < b1; ++b) s += block_counts[b];
    part[tid] = s;
    __syncthreads();
    // Hillis-Steele inclusive scan over 1024 partials
    for (int off = 1; off < 1024; off <<= 1) {
        long long v = (tid >= off) ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    long long run = part[tid] - s;  // exclusive prefix of this lane's range
    for (int b = b0; b < b1; ++b) {
        const int32_t cnt = block_counts[b];
        block_counts[b] = (int32_t)run;
        run += cnt;
    }
    if (tid == 1023) *total = part[1023];
}

// SELF_SCAN (few thousand workgroups at most): `block_offsets` holds the raw per-workgroup COUNTS and every workgroup sums the counts before
// its own by itself (a few KB out of L2) — the single-workgroup scan launch between count and scatter goes away (three launches -> two);
// the last workgroup writes the total.
template <bool SELF_SCAN>
__global__ void __launch_bounds__(kBlock)
compact_scatter_kernel(const uint8_t* __restrict__ mask, int64_t n, const int32_t* __restrict__ block_offsets,
                       int32_t* __restrict__ index, long long* __restrict__ total) {
    __shared__ int wsum[kBlock / kWave];
    __shared__ long long before_s;
    long long before = 0;
    if (SELF_SCAN) {
        __shared__ unsigned long long psum[kBlock / kWave];
        unsigned long long mine = 0;
        for (int b = threadIdx.x; b < (int)blockIdx.x; b += kBlock) mine += (unsigned long long)block_offsets[b];
        mine = wave_sum(mine);
        if ((threadIdx.x & (kWave - 1)) == 0) psum[threadIdx.x / kWave] = mine;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long t = 0;
            for (int i = 0; i < kBlock / kWave; ++i) t += psum[i];
            before_s = (long long)t;
            if (blockIdx.x == gridDim.x - 1) *total = (long long)t + block_offsets[blockIdx.x];
        }
        __syncthreads();
        before = before_s;
    } else {
        before = block_offsets[blockIdx.x];
    }
    uint32_t bits;
    const int64_t base = (int64_t)blockIdx.x * kChunk + (int64_t)threadIdx.x * kPerLane;
    const int cnt = lane_count(mask, base, n, bits);
    // inclusive wave scan by shuffles
    const int lane = threadIdx.x & (kWave - 1);
    int incl = cnt;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const int v = __shfl_up(incl, off, kWave);
        if (lane >= off) incl += v;
    }
    if (lane == kWave - 1) wsum[threadIdx.x / kWave] = incl;
    __syncthreads();
    int wave_base = 0;
    for (int i = 0; i < (int)(threadIdx.x / kWave); ++i) wave_base += wsum[i];
    int64_t o = (int64_t)before + wave_base + (incl - cnt);
    while (bits) {
        const int e = __ffs(bits) - 1;
        bits &= bits - 1;
        index[o++] = (int32_t)(base + e);
    }
}

static unsigned grid_for(int64_t items) {
    int64_t b = (items + kBlock - 1) / kBlock;
    if (b > kStreamGrid) b = kStreamGrid;
    if (b < 1) b = 1;
    return (unsigned)b;
}

}  // namespace atx

using namespace atx;

extern "C" int atx_mask_build(const void* m, int64_t m_stride, uint8_t* mask, int64_t n, int cmp, double threshold,
                              int dtype, void* stream) {
    ATX_REQUIRE((m && mask) || n == 0, ATX_EINVAL, "atx_mask_build: null pointer");
    ATX_REQUIRE(n >= 0 && m_stride >= 1, ATX_EINVAL, "atx_mask_build: bad n=%lld / stride=%lld", (long long)n, (long long)m_stride);
    ATX_REQUIRE(cmp >= ATX_CMP_GT && cmp <= ATX_CMP_ISNAN, ATX_EINVAL, "atx_mask_build: bad comparison %d", cmp);
    ATX_REQUIRE(dtype == ATX_F32 || dtype == ATX_F64, ATX_EINVAL, "atx_mask_build: bad dtype %d", dtype);
    ATX_REQUIRE((reinterpret_cast<uintptr_t>(mask) & 3u) == 0, ATX_EALIGN, "atx_mask_build: mask must be 4-byte aligned");
    if (n == 0) return ATX_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned g = grid_for((n + 3) / 4);
    if (dtype == ATX_F32)
        hipLaunchKernelGGL(mask_build_kernel<float>, dim3(g), dim3(kBlock), 0, s, static_cast<const float*>(m), m_stride, mask, n, cmp, (float)threshold);
    else
        hipLaunchKernelGGL(mask_build_kernel<double>, dim3(g), dim3(kBlock), 0, s, static_cast<const double*>(m), m_stride, mask, n, cmp, threshold);
    ATX_LAUNCH_CHECK("mask_build");
    return ATX_OK;
}

extern "C" int atx_mask_count(const uint8_t* mask, int64_t n, int64_t* count, void* stream) {
    ATX_REQUIRE(count && (mask || n == 0), ATX_EINVAL, "atx_mask_count: null pointer");
    ATX_REQUIRE(n >= 0, ATX_EINVAL, "atx_mask_count: negative n");
    hipStream_t s = static_cast<hipStream_t>(stream);
    int st = hip_status(hipMemsetAsync(count, 0, sizeof(int64_t), s), "atx_mask_count memset");
    if (st != ATX_OK) return st;
    if (n == 0) return ATX_OK;
    const unsigned count_grid = grid_for(n) > 2048u ? 2048u : grid_for(n);  // one atomic per wave on one address: keep them few
    hipLaunchKernelGGL(mask_count_kernel, dim3(count_grid), dim3(kBlock), 0, s, mask, n, reinterpret_cast<unsigned long long*>(count));
    ATX_LAUNCH_CHECK("mask_count");
    return ATX_OK;
}

extern "C" size_t atx_mask_to_index_workspace(int64_t n) {
    if (n < 0) return 0;
    const int64_t n_blocks = (n + kChunk - 1) / kChunk;
    return (size_t)((n_blocks + 1) * sizeof(int32_t) + 15) & ~size_t(15);
}

extern "C" int atx_mask_to_index(const uint8_t* mask, int64_t n, int32_t* index, int64_t* count, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    ATX_REQUIRE(count && workspace && ((mask && index) || n == 0), ATX_EINVAL, "atx_mask_to_index: null pointer");
    ATX_REQUIRE(n >= 0 && n <= INT32_MAX, ATX_EINVAL, "atx_mask_to_index: n=%lld outside int32", (long long)n);
    ATX_REQUIRE(workspace_bytes >= atx_mask_to_index_workspace(n), ATX_EWORKSPACE, "atx_mask_to_index: workspace %zu < %zu",
                workspace_bytes, atx_mask_to_index_workspace(n));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n == 0) return hip_status(hipMemsetAsync(count, 0, sizeof(int64_t), s), "atx_mask_to_index memset");
    const int n_blocks = (int)((n + kChunk - 1) / kChunk);
    int32_t* block_counts = static_cast<int32_t*>(workspace);
    hipLaunchKernelGGL(compact_count_kernel, dim3(n_blocks), dim3(kBlock), 0, s, mask, n, block_counts);
    ATX_LAUNCH_CHECK("compact_count");
    constexpr int kCompactSelfScan = 4096;  // workgroups up to which the scatter sums the counts before it by itself (16 M points)
    if (n_blocks <= kCompactSelfScan) {
        hipLaunchKernelGGL(compact_scatter_kernel<true>, dim3(n_blocks), dim3(kBlock), 0, s, mask, n, block_counts, index, reinterpret_cast<long long*>(count));
        ATX_LAUNCH_CHECK("compact_scatter");
        return ATX_OK;
    }
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(1024), 0, s, block_counts, n_blocks, reinterpret_cast<long long*>(count));
    ATX_LAUNCH_CHECK("compact_scan");
    hipLaunchKernelGGL(compact_scatter_kernel<false>, dim3(n_blocks), dim3(kBlock), 0, s, mask, n, block_counts, index, nullptr);
    ATX_LAUNCH_CHECK("compact_scatter");
    return ATX_OK;
}
