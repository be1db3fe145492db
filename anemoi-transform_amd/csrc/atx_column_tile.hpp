// What a "workgroup per tile of consecutive points, columns staged in LDS" kernel needs (atx_levels.hip, atx_geopotential.hip).  In
// ATX_COLUMNS the columns of PT consecutive points are ONE run of PT x pitch elements: the lanes copy it into LDS in order
// (stage_columns), 16 bytes per lane where the stack allows (column_route), and no lane walks a column in HBM.  PT is what the LDS
// budget holds (tile_points) of the kernel's own carve struct.  The pressures of the hybrid levels are here too, in one spelling.
#pragma once

#include "atx_common.hpp"

namespace atx {

constexpr int kTileBlock = 256;                     // lanes per workgroup
constexpr int kTileMaxPoints = 256;                 // points per tile at most: a phase with one lane per point is one pass of the block
// Five workgroups share the 160 KiB of a CU: one's narrow phases (a lane per point) hide behind the others' loads (the geopotential
// kernel at O1280 x 137, float32 / float64: 64 KiB 8.77 / 10.20 ms, 16 KiB 7.37 / 6.91 ms, 32 KiB 7.23 / 6.73 ms in the same run).
constexpr int64_t kTileLdsPreferred = 32 * 1024;
constexpr int64_t kTileLdsLimit = 64 * 1024;         // what one workgroup may ask for, where a single point does not fit the above

__host__ __device__ inline int64_t round16(int64_t bytes) { return (bytes + 15) / 16 * 16; }

// The points of a tile: as many as the preferred LDS budget holds (at most kTileMaxPoints), one at least if the limit holds it; 0: not
// even one.  `bytes(pt)`: the LDS of a tile of pt points, growing with pt.
template <typename Bytes>
static int tile_points(Bytes&& bytes) {
    for (const int64_t budget : {kTileLdsPreferred, kTileLdsLimit}) {
        int pt = 0;
        for (int step = kTileMaxPoints; step > 0; step /= 2)  // the largest pt <= kTileMaxPoints that fits
            if (pt + step <= kTileMaxPoints && bytes((int64_t)(pt + step)) <= budget) pt += step;
        if (pt > 0) return pt;
    }
    return 0;
}

// How a stack's columns are staged: 16 bytes per lane where base and pitch keep every vector aligned and a column's last vector ends
// inside the pitch — lds_pitch, the elements between two points' columns in LDS, is then `rows` rounded up to whole vectors.
struct ColumnRoute { bool vector; int lds_pitch; };
template <int VEC>
inline ColumnRoute column_route(const void* base, int64_t pitch, int rows) {
    const int covered = (rows + VEC - 1) / VEC * VEC;
    const bool vector = aligned16(base) && pitch % VEC == 0 && covered <= pitch;
    return {vector, vector ? covered : rows};
}

// Item i = tid, tid + kTileBlock, ... of a [rows][width] tile as (row, col) = (i / width, i % width): ONE division per lane and loop,
// then steps of (kTileBlock / width, kTileBlock % width) with a carry — a division per item cost as much as a third of a logarithm.
struct TileWalk {
    int row, col, width, step_row, step_col;
    __device__ __forceinline__ TileWalk(int tid, int w) : width(w) {
        row = tid / w;
        col = tid - row * w;
        step_row = kTileBlock / w;
        step_col = kTileBlock - step_row * w;
    }
    __device__ __forceinline__ void next() {
        row += step_row;
        col += step_col;
        if (col >= width) {
            col -= width;
            ++row;
        }
    }
};

// The columns of the tile's npt points (from point p0, `pitch` apart in src) into xs, lds_pitch apart: V, lds_pitch as column_route says.
template <typename T, int V>
__device__ __forceinline__ void stage_columns(const T* __restrict__ src, T* __restrict__ xs, int64_t p0, int npt, int64_t pitch, int lds_pitch, int tid) {
    const int C = lds_pitch / V;
    TileWalk w(tid, C);
    for (int i = tid; i < npt * C; i += kTileBlock, w.next()) {
        const int pt = w.row, c = w.col;
        const Pack<T, V> v = pw_load_nt<T, V>(src + (p0 + pt) * pitch + (int64_t)c * V);
        *reinterpret_cast<Pack<T, V>*>(xs + (int64_t)pt * lds_pitch + c * V) = v;
    }
}

// Hybrid levels: the pressure of half level j and of full level j (between the half levels j and j + 1) under the surface pressure sp,
// one float64 operation at a time (-ffp-contract=off).  A and B may be the tables in global memory or a copy in LDS.
__device__ __forceinline__ double half_level(const double* A, const double* B, int j, double sp) { return A[j] + B[j] * sp; }
__device__ __forceinline__ double full_level(const double* A, const double* B, int j, double sp) {
    return (half_level(A, B, j, sp) + half_level(A, B, j + 1, sp)) / 2.0;
}

}  // namespace atx
