// Point location in a triangulated set of source points on the unit sphere: atx_mesh_locate (include/atx_mesh.h).
//
// interp.locate_walk_host is the statement; interp.locate_brute_host states the answer again without a walk.  The loop uses only
// *, +, -, /, comparisons and table reads, and the build has no contraction (-ffp-contract=off), so what this kernel writes equals
// the host statement bit for bit (tests/test_gpu_mesh_locate.py).  The hull that gives the triangles stays on the host, in Qhull.
//
// One target per lane.  A lane holds its target and walks from its seed: at every triangle it reads the three vertex numbers and, if
// it has to move on, the three neighbours (24 bytes of tables) and the three vertices (72 bytes), all at addresses that depend on the
// step before, so a move costs a round trip to memory and the lanes of a wave wait for its longest walk.  Targets in grid order make
// neighbouring lanes read the same triangles.  None of this has been measured beyond tools/linear_unstructured_bench.py.
//
// Launch shape, as atx_plan_box_average.hip: 256-lane workgroups, a grid-stride loop under a grid cap, 64-bit target counters.  No
// atomics, no LDS; plain vector stores.  Whatever tri, nbr and seed hold, every read stays inside the arrays as sized by the arguments:
// a triangle number is checked against n_tri and a vertex number against n_src before it is used, and a lane that fails the check
// stops with status 3.  The walk is bounded by max_steps, which the entry point caps.
#include <cmath>

#include "../../../include/atx_mesh.h"
#include "../atx_host.hpp"

namespace atx_mesh {

constexpr int kBlock = 256;  // 4 waves: one per SIMD of a CU
constexpr int kGrid = 2048;  // grid cap: beyond 2^19 targets a lane takes further targets

enum : int32_t { kFound = 0, kUndecided = 1, kOutside = 2, kMalformed = 3 };

struct Vec {
    double x, y, z;
};

__device__ __forceinline__ Vec load_vec(const double* __restrict__ xyz, int64_t i) { return Vec{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]}; }

// The determinant of include/atx_mesh.h: every operation rounded on its own, the sum taken left to right.
__device__ __forceinline__ double det(const Vec& p, const Vec& b, const Vec& c) {
    const double cx = b.y * c.z - b.z * c.y;
    const double cy = b.z * c.x - b.x * c.z;
    const double cz = b.x * c.y - b.y * c.x;
    return (p.x * cx + p.y * cy) + p.z * cz;
}

__global__ __launch_bounds__(kBlock) void locate_kernel(const double* __restrict__ src_xyz, int64_t n_src, const int32_t* __restrict__ tri,
                                                         const int32_t* __restrict__ nbr, const uint8_t* __restrict__ flag, int64_t n_tri,
                                                         const double* __restrict__ tgt_xyz, const int32_t* __restrict__ seed, int64_t n_tgt,
                                                         int32_t max_steps, int32_t* __restrict__ tri_out, double* __restrict__ w,
                                                         int32_t* __restrict__ status, int32_t* __restrict__ steps) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_tgt; i += stride) {
        const Vec p = load_vec(tgt_xyz, i);
        int64_t t = seed[i];
        int32_t moves = 0, verdict;
        double w0 = 0.0, w1 = 0.0, w2 = 0.0;
        for (;;) {
            if (t < 0 || t >= n_tri) {
                verdict = kMalformed;
                break;
            }
            if (flag[t] != 0) {
                verdict = kOutside;
                break;
            }
            const int64_t ia = tri[3 * t], ib = tri[3 * t + 1], ic = tri[3 * t + 2];
            if (ia < 0 || ia >= n_src || ib < 0 || ib >= n_src || ic < 0 || ic >= n_src) {
                verdict = kMalformed;
                break;
            }
            const Vec a = load_vec(src_xyz, ia), b = load_vec(src_xyz, ib), c = load_vec(src_xyz, ic);
            double d0 = det(p, b, c), d1 = det(p, c, a), d2 = det(p, a, b);
            const double tol = -0x1p-30 * det(a, b, c);
            if (d0 >= tol && d1 >= tol && d2 >= tol) {
                d0 = d0 < 0.0 ? 0.0 : d0;
                d1 = d1 < 0.0 ? 0.0 : d1;
                d2 = d2 < 0.0 ? 0.0 : d2;
                const double sum = (d0 + d1) + d2;
                w0 = d0 / sum;
                w1 = d1 / sum;
                w2 = d2 / sum;
                verdict = kFound;
                break;
            }
            if (moves >= max_steps) {
                verdict = kUndecided;
                break;
            }
            int e = 0;  // the first of the smallest d_i
            double least = d0;
            if (d1 < least) {
                e = 1;
                least = d1;
            }
            if (d2 < least) e = 2;
            t = nbr[3 * t + e];
            ++moves;
        }
        if (verdict == kMalformed) {
            t = -1;
            w0 = w1 = w2 = __builtin_nan("");
        }
        tri_out[i] = (int32_t)t;
        w[3 * i] = w0;
        w[3 * i + 1] = w1;
        w[3 * i + 2] = w2;
        status[i] = verdict;
        steps[i] = moves;
    }
}

}  // namespace atx_mesh

extern "C" int atx_mesh_version(void) { return ATX_MESH_VERSION; }

extern "C" const char* atx_mesh_last_error(void) { return atx::last_error().c_str(); }

extern "C" int atx_mesh_locate(const double* src_xyz, int64_t n_src, const int32_t* tri, const int32_t* nbr, const uint8_t* flag,
                               int64_t n_tri, const double* tgt_xyz, const int32_t* seed, int64_t n_tgt, int32_t max_steps,
                               int32_t* tri_out, double* w, int32_t* status, int32_t* steps, void* stream) {
    using namespace atx_mesh;
    const char* fn = "atx_mesh_locate";
    constexpr int64_t kMax = 2147483647;
    ATX_REQUIRE(n_src >= 1 && n_src <= kMax && n_tri >= 1 && n_tri <= kMax, ATX_EINVAL,
                "%s: n_src = %lld, n_tri = %lld: a size is outside 1 .. 2^31 - 1", fn, (long long)n_src, (long long)n_tri);
    ATX_REQUIRE(n_tgt >= 0 && n_tgt <= kMax, ATX_EINVAL, "%s: n_tgt = %lld is outside 0 .. 2^31 - 1", fn, (long long)n_tgt);
    ATX_REQUIRE(max_steps >= 0 && max_steps <= ATX_MESH_MAX_STEPS, ATX_EINVAL, "%s: max_steps = %d is outside 0 .. %d", fn, (int)max_steps,
                (int)ATX_MESH_MAX_STEPS);
    if (n_tgt == 0) return ATX_OK;
    ATX_REQUIRE(src_xyz && tri && nbr && flag && tgt_xyz && seed && tri_out && w && status && steps, ATX_EINVAL,
                "%s: null pointer (src_xyz=%p tri=%p nbr=%p flag=%p tgt_xyz=%p seed=%p tri_out=%p w=%p status=%p steps=%p) with n_tgt = %lld",
                fn, (const void*)src_xyz, (const void*)tri, (const void*)nbr, (const void*)flag, (const void*)tgt_xyz, (const void*)seed,
                (void*)tri_out, (void*)w, (void*)status, (void*)steps, (long long)n_tgt);
    hipLaunchKernelGGL(locate_kernel, dim3(atx::grid_for(n_tgt, kBlock, kGrid)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), src_xyz, n_src, tri, nbr,
                       flag, n_tri, tgt_xyz, seed, n_tgt, max_steps, tri_out, w, status, steps);
    ATX_LAUNCH_CHECK(fn);
    return ATX_OK;
}
