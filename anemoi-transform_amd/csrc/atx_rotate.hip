// Vector frames: the (x, y) components of a vector field on a grid, mapped from one projection's frame to another's.
//
// rotate_winds / unrotate_winds (R: filters/fields/rotate_winds.py:61-118, earthkit-geo's rotate_vector) apply, at every grid
// point, a 2x2 map that depends on where the point is, never on the level: the host builds it once per grid and projection pair
// (projections.py, float64, cast to the stack's dtype) and every level of the two stacks shares it.  The statement, per element,
// in the stack's dtype and without contraction (the library is built with -ffp-contract=off), is that of atx.h:
//
//   ATX_FRAME_ROTATION  frame[p] = (c, s):             (c u - s v,  s u + c v)
//   ATX_FRAME_GENERAL   frame[p] = (m00, m01, m10, m11): mx = m00 u + m01 v,  my = m10 u + m11 v,
//                                                        k = sqrt(u u + v v) / sqrt(mx mx + my my),  (mx k, my k)
//   u == v == 0: the input, signed zeros kept.
//
// Access patterns — two stacks in, two out, plus the frame table (algorithmic bytes 4 N L B + N F B):
//   ATX_COLUMNS  one 16-byte vector (VEC levels of one point) per lane and slot, as atx_combine_stack does; the lanes of a point
//                read the same frame words, which costs one request.  Data loads and stores are non-temporal (read once).
//   ATX_FIELDS   one lane per point, its frame in registers, a chunk of kLevChunk levels per grid.y: the frame costs at most
//                F / (4 kLevChunk) of the data bytes.  Each level of a wave's 64 points is one coalesced run.
// Every lane loads all its operands before it stores anything, so x_out == x and y_out == y (in place) are safe without restrict.
#include "atx_common.hpp"

namespace atx {

constexpr int kRotSlots = 2;   // COLUMNS: 16-byte vectors per lane (loads of both in flight before the first store)
constexpr int kLevChunk = 16;  // FIELDS: levels per grid.y
constexpr int kLevBatch = 8;   // FIELDS: levels loaded per lane before the batch is stored

template <typename T, int KIND>
__device__ __forceinline__ void rotate_one(const T* f, T u, T v, T& x, T& y) {
    if constexpr (KIND == ATX_FRAME_ROTATION) {
        x = f[0] * u - f[1] * v;
        y = f[1] * u + f[0] * v;
    } else {
        const T mx = f[0] * u + f[1] * v;
        const T my = f[2] * u + f[3] * v;
        const T k = sqrt(u * u + v * v) / sqrt(mx * mx + my * my);
        x = mx * k;
        y = my * k;
    }
    if (u == T(0) && v == T(0)) {
        x = u;
        y = v;
    }
}

template <int KIND>
constexpr int frame_width() {
    return KIND == ATX_FRAME_ROTATION ? 2 : 4;
}

// the F words of one point's frame (the table is 16-byte aligned and F * sizeof(T) is 8, 16 or 32 bytes)
template <typename T, int F>
__device__ __forceinline__ void load_frame(const T* __restrict__ frame, int64_t p, T* f) {
    if constexpr (F * sizeof(T) == 8) {
        typedef T NV __attribute__((ext_vector_type(2)));
        const NV a = *reinterpret_cast<const NV*>(frame + p * F);
        f[0] = a[0];
        f[1] = a[1];
    } else {
        typedef T NV __attribute__((ext_vector_type(16 / sizeof(T))));
        constexpr int N = 16 / sizeof(T);
#pragma unroll
        for (int h = 0; h < F / N; ++h) {
            const NV a = *reinterpret_cast<const NV*>(frame + p * F + h * N);
#pragma unroll
            for (int j = 0; j < N; ++j) f[h * N + j] = a[j];
        }
    }
}

template <typename T, int N>
__device__ __forceinline__ Pack<T, N> nt_load(const T* p) {
    if constexpr (N > 1) {
        typedef T NV __attribute__((ext_vector_type(N)));
        NV v = __builtin_nontemporal_load(reinterpret_cast<const NV*>(p));
        return *reinterpret_cast<Pack<T, N>*>(&v);
    } else {
        Pack<T, 1> r;
        r.v[0] = __builtin_nontemporal_load(p);
        return r;
    }
}

template <typename T, int N>
__device__ __forceinline__ void nt_store(T* p, const Pack<T, N>& v) {
    if constexpr (N > 1) {
        typedef T NV __attribute__((ext_vector_type(N)));
        __builtin_nontemporal_store(*reinterpret_cast<const NV*>(&v), reinterpret_cast<NV*>(p));
    } else {
        __builtin_nontemporal_store(v.v[0], p);
    }
}

// ATX_COLUMNS: the stack as n_pts rows of pitch / VEC vectors; vector i of the grid is (point i / vpr, levels (i % vpr) * VEC ..)
template <typename T, int VEC, int KIND, typename I>
__global__ void __launch_bounds__(kBlock)
rotate_columns_kernel(const T* x, const T* y, T* xo, T* yo, const T* __restrict__ frame, I total, I vpr, int n_lev) {
    constexpr int F = frame_width<KIND>();
    const I base = (I)blockIdx.x * (I)(kBlock * kRotSlots) + (I)threadIdx.x;
    Pack<T, VEC> a[kRotSlots], b[kRotSlots];
    T f[kRotSlots][F];
    I point[kRotSlots];
#pragma unroll
    for (int s = 0; s < kRotSlots; ++s) {
        const I i = base + (I)(s * kBlock);
        if (i < total) {
            a[s] = nt_load<T, VEC>(x + (int64_t)i * VEC);
            b[s] = nt_load<T, VEC>(y + (int64_t)i * VEC);
            point[s] = i / vpr;
            load_frame<T, F>(frame, (int64_t)point[s], f[s]);
        }
    }
#pragma unroll
    for (int s = 0; s < kRotSlots; ++s) {
        const I i = base + (I)(s * kBlock);
        if (i >= total) continue;
        const int col = (int)(i - point[s] * vpr) * VEC;
        Pack<T, VEC> ox, oy;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            T rx, ry;
            rotate_one<T, KIND>(f[s], a[s].v[e], b[s].v[e], rx, ry);
            const bool live = col + e < n_lev;
            ox.v[e] = live ? rx : T(0);  // padding is written with zeros
            oy.v[e] = live ? ry : T(0);
        }
        nt_store<T, VEC>(xo + (int64_t)i * VEC, ox);
        nt_store<T, VEC>(yo + (int64_t)i * VEC, oy);
    }
}

// ATX_FIELDS: lane = point (padding points p in [n_pts, pitch) written with zeros), grid.y = chunk of kLevChunk levels
template <typename T, int KIND>
__global__ void __launch_bounds__(kBlock)
rotate_fields_kernel(const T* x, const T* y, T* xo, T* yo, const T* __restrict__ frame, int64_t n_pts, int n_lev, int64_t pitch) {
    constexpr int F = frame_width<KIND>();
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= pitch) return;
    const bool live = p < n_pts;
    T f[F];
    if (live) load_frame<T, F>(frame, p, f);
    const int l0 = (int)blockIdx.y * kLevChunk;
    const int l1 = l0 + kLevChunk < n_lev ? l0 + kLevChunk : n_lev;
    for (int lb = l0; lb < l1; lb += kLevBatch) {
        T u[kLevBatch], v[kLevBatch];
#pragma unroll
        for (int j = 0; j < kLevBatch; ++j) {
            if (lb + j < l1) {
                const int64_t i = (int64_t)(lb + j) * pitch + p;
                u[j] = __builtin_nontemporal_load(x + i);
                v[j] = __builtin_nontemporal_load(y + i);
            }
        }
#pragma unroll
        for (int j = 0; j < kLevBatch; ++j) {
            if (lb + j < l1) {
                T rx = T(0), ry = T(0);
                if (live) rotate_one<T, KIND>(f, u[j], v[j], rx, ry);
                const int64_t i = (int64_t)(lb + j) * pitch + p;
                __builtin_nontemporal_store(rx, xo + i);
                __builtin_nontemporal_store(ry, yo + i);
            }
        }
    }
}

template <typename T, int KIND>
static int rotate_typed(const void* x, const void* y, void* xo, void* yo, const void* frame, int64_t n_pts, int n_lev, int64_t pitch,
                        int layout, hipStream_t st) {
    const T* xx = static_cast<const T*>(x);
    const T* yy = static_cast<const T*>(y);
    T* ox = static_cast<T*>(xo);
    T* oy = static_cast<T*>(yo);
    const T* ff = static_cast<const T*>(frame);
    if (layout == ATX_FIELDS) {
        const dim3 grid((unsigned)((pitch + kBlock - 1) / kBlock), (unsigned)((n_lev + kLevChunk - 1) / kLevChunk));
        hipLaunchKernelGGL((rotate_fields_kernel<T, KIND>), grid, dim3(kBlock), 0, st, xx, yy, ox, oy, ff, n_pts, n_lev, pitch);
    } else {
        constexpr int VEC = Vec16<T>::N;
        const bool vec_ok = pitch % VEC == 0 && aligned16(x) && aligned16(y) && aligned16(xo) && aligned16(yo);
        const int vec = vec_ok ? VEC : 1;
        const int64_t vpr = pitch / vec, total = n_pts * vpr;
        const int64_t blocks = (total + kBlock * kRotSlots - 1) / (kBlock * kRotSlots);
        const bool small = total < (int64_t)UINT32_MAX - kBlock * kRotSlots;  // 32-bit index arithmetic (the division by vpr)
#define ATX_ROT_LAUNCH(V_, I_)                                                                                                      \
    hipLaunchKernelGGL((rotate_columns_kernel<T, V_, KIND, I_>), dim3((unsigned)blocks), dim3(kBlock), 0, st, xx, yy, ox, oy, ff, \
                       (I_)total, (I_)vpr, n_lev)
        if (vec_ok && small) ATX_ROT_LAUNCH(VEC, uint32_t);
        else if (vec_ok) ATX_ROT_LAUNCH(VEC, int64_t);
        else if (small) ATX_ROT_LAUNCH(1, uint32_t);
        else ATX_ROT_LAUNCH(1, int64_t);
#undef ATX_ROT_LAUNCH
    }
    ATX_LAUNCH_CHECK("rotate_vectors_stack");
    return ATX_OK;
}

}  // namespace atx

using namespace atx;

extern "C" int atx_rotate_vectors_stack(const void* x, const void* y, void* x_out, void* y_out, const void* frame, int frame_kind,
                                        int64_t n_pts, int64_t n_lev, int64_t pitch, int dtype, int layout, void* stream) {
    ATX_REQUIRE((x && y && x_out && y_out && frame) || n_pts == 0, ATX_EINVAL, "atx_rotate_vectors_stack: null pointer");
    ATX_REQUIRE(frame_kind == ATX_FRAME_ROTATION || frame_kind == ATX_FRAME_GENERAL, ATX_EINVAL,
                "atx_rotate_vectors_stack: bad frame kind %d", frame_kind);
    ATX_REQUIRE(dtype == ATX_F32 || dtype == ATX_F64, ATX_EINVAL, "atx_rotate_vectors_stack: bad dtype %d", dtype);
    ATX_REQUIRE(layout == ATX_COLUMNS || layout == ATX_FIELDS, ATX_EINVAL, "atx_rotate_vectors_stack: bad layout %d", layout);
    ATX_REQUIRE(n_pts >= 0 && n_lev > 0 && n_lev < INT32_MAX, ATX_EINVAL, "atx_rotate_vectors_stack: bad sizes");
    ATX_REQUIRE(pitch >= (layout == ATX_COLUMNS ? n_lev : n_pts), ATX_ESHAPE, "atx_rotate_vectors_stack: pitch %lld too small",
                (long long)pitch);
    ATX_REQUIRE(x_out != y_out || n_pts == 0, ATX_EINVAL, "atx_rotate_vectors_stack: x_out and y_out are the same buffer");
    ATX_REQUIRE(aligned16(frame), ATX_EALIGN, "atx_rotate_vectors_stack: the frame table must be 16-byte aligned");
    if (n_pts == 0) return ATX_OK;
    ATX_REQUIRE(layout == ATX_COLUMNS || (pitch + kBlock - 1) / kBlock < 0x7fffffffll, ATX_EINVAL, "atx_rotate_vectors_stack: too many points");
    ATX_REQUIRE(layout == ATX_FIELDS || n_pts * pitch / (kBlock * kRotSlots) < 0x7fffffffll, ATX_EINVAL,
                "atx_rotate_vectors_stack: stack too large");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int L = (int)n_lev;
    if (dtype == ATX_F32) {
        if (frame_kind == ATX_FRAME_ROTATION) return rotate_typed<float, ATX_FRAME_ROTATION>(x, y, x_out, y_out, frame, n_pts, L, pitch, layout, s);
        return rotate_typed<float, ATX_FRAME_GENERAL>(x, y, x_out, y_out, frame, n_pts, L, pitch, layout, s);
    }
    if (frame_kind == ATX_FRAME_ROTATION) return rotate_typed<double, ATX_FRAME_ROTATION>(x, y, x_out, y_out, frame, n_pts, L, pitch, layout, s);
    return rotate_typed<double, ATX_FRAME_GENERAL>(x, y, x_out, y_out, frame, n_pts, L, pitch, layout, s);
}
