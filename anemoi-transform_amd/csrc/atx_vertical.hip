// Vertical reductions over the model levels of each grid point: the pressure at a height above the ground.
//
// Every other kernel of the library works per level (pointwise, combine) or horizontally (gather).  This one walks each column
// of two model-level stacks (temperature, specific humidity), bottom level first, and reduces it to one value per point:
// earthkit-meteo's vertical.pressure_at_height_levels(height, t, q, sp, A, B) with alpha_top="ifs", the arithmetic of
// R: filters/fields/q_height.py:203-213 / :416-426 (earthkit-meteo is absent here; the statement is restated in
// tests/vertical_restatement.py and pinned by the reference's 2 m dewpoint vectors only).  Levels k = 0 .. n-1, top first;
// A and B hold the n+1 half-level coefficients:
//
//   p_half[k] = A[k] + B[k] sp                      alpha[0] = ln 2,  alpha[k] = 1 - p_half[k] / (p_half[k+1] - p_half[k]) ln(p_half[k+1] / p_half[k])
//   p_full[k] = (p_half[k] + p_half[k+1]) / 2       dphi[k]  = sum_{j = n-1 .. k} alpha[j] R(q_j) t_j,  R(q) = Rd (1 - q) + Rv q
//   i = #{k : g h > dphi[k]}      i == 0: p = p_half[n] + g h / dphi[n-1] (p_full[n-1] - p_half[n])
//                                 i >  0: a = n - i - 1 (-1 wraps to n - 1, as numpy's index does), b = a + 1,
//                                         p = p_full[b] + (g h - dphi[b]) / (dphi[a] - dphi[b]) (p_full[a] - p_full[b])
//
// Everything is evaluated in float64 for both widths, statement by statement in numpy's order (IEEE divisions, no contraction,
// the library's <= 1 ulp atx_log), so the float64 result follows the restatement to a few ulps; alpha is ill-conditioned
// (1 - x with x ~ 0.999 near the ground), and one ulp of a logarithm moves it by ~1e-13 relative, which the interpolation then
// damps.  delta[0] = ln(p_half[1] / 0.1) of the statement feeds nothing once alpha[0] = ln 2: it is not computed.
//
// The count i runs over the WHOLE column (a NaN or a non-physical value above the height changes it), so every column is walked
// to the top; there is no early exit.  The interpolation needs dphi at two levels that are known only at the end: the walk keeps
// the pair at the first level that does not count while all levels below it did — which IS the pair for every column whose dphi
// grows upward, NaN columns included — and the rare column where it is not (dphi decreasing somewhere: negative temperatures or
// coefficients) walks again from the bottom to level a.
//
// Access patterns (one lane per point, a 256-lane workgroup per 256 consecutive points):
//   ATX_FIELDS   level k of the wave's 64 points is one contiguous run: a coalesced load per level and stack.
//   ATX_COLUMNS  each point's levels are contiguous: per-lane 16-byte loads (4 float32 / 2 float64 levels), bottom group first.
//                Chosen for simplicity: the wave's 64 columns are one contiguous run of 64 x pitch elements, so every line is used
//                whole — but through L2 only, and each load instruction touches 64 lines.  Measured at O1280 x 137 it runs at a
//                third of the FIELDS rate ("Column kernel"); a cooperative LDS tile (a wave loads 64-byte runs of
//                16 columns per instruction) is the next step for this layout.
#include "atx_common.hpp"

namespace atx {

constexpr double kRd = 287.0597, kRv = 461.5250;  // J / (kg K): the epsilon constants of the humidity operators
constexpr double kGravity = 9.80665;
constexpr double kLn2 = 0.69314718055994530942;

// alpha[k] R(q) t of one level (the term dphi accumulates)
__device__ __forceinline__ double layer_thickness(const double* __restrict__ A, const double* __restrict__ B, int k, double sp,
                                                  double t, double q) {
    double alpha = kLn2;  // alpha_top = "ifs"
    if (k > 0) {  // (uniform: every lane of the wave is at the same level)
        const double lo = A[k] + B[k] * sp, hi = A[k + 1] + B[k + 1] * sp;
        const double delta = atx_log(hi / lo);
        alpha = 1.0 - lo / (hi - lo) * delta;
    }
    const double r = kRd * (1.0 - q) + kRv * q;
    return alpha * r * t;
}

__device__ __forceinline__ double full_level(const double* __restrict__ A, const double* __restrict__ B, int k, double sp) {
    return ((A[k] + B[k] * sp) + (A[k + 1] + B[k + 1] * sp)) / 2.0;
}

// the running state of one column's walk
struct ColumnWalk {
    double dphi = 0.0;    // dphi of the level last walked
    double bottom = 0.0;  // dphi[n-1]
    double da = 0.0, db = 0.0;  // dphi[a0], dphi[a0 + 1]
    int count = 0;        // #{walked k : g h > dphi[k]}
    int a0 = -1;

    __device__ __forceinline__ void step(int k, int n, double term, double tdphi) {
        const bool all_below = count == n - 1 - k;
        const double next = dphi + term;
        if (k == n - 1) bottom = next;
        if (all_below && k < n - 1) {
            da = next;
            db = dphi;
            a0 = k;
        }
        dphi = next;
        count += tdphi > next ? 1 : 0;
    }
};

template <typename T>
__device__ __forceinline__ T at(const T* base, int64_t i) {
    return __builtin_nontemporal_load(base + i);  // every element is read once
}

// COLUMNS: VEC levels per 16-byte load (1: scalar loads, for a pitch or base that is not 16-byte aligned)
template <typename T, int LAYOUT, int VEC>
__global__ void __launch_bounds__(kBlock)
pressure_at_height_kernel(const T* __restrict__ t, const T* __restrict__ q, const T* __restrict__ sp_in, const double* __restrict__ A,
                          const double* __restrict__ B, int64_t n_pts, int n, int64_t pitch, double tdphi, T* __restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n_pts) return;
    const double sp = (double)sp_in[p];
    ColumnWalk w;
    if constexpr (LAYOUT == ATX_FIELDS) {
#pragma unroll 4
        for (int k = n - 1; k >= 0; --k) {
            const double tk = (double)at(t, (int64_t)k * pitch + p), qk = (double)at(q, (int64_t)k * pitch + p);
            w.step(k, n, layer_thickness(A, B, k, sp, tk, qk), tdphi);
        }
    } else {
        const T* tc = t + p * pitch;
        const T* qc = q + p * pitch;
        for (int g = (n - 1) / VEC; g >= 0; --g) {
            Pack<T, VEC> tv, qv;
            if constexpr (VEC > 1) {
                typedef T NV __attribute__((ext_vector_type(VEC)));
                NV a = __builtin_nontemporal_load(reinterpret_cast<const NV*>(tc + g * VEC));
                NV b = __builtin_nontemporal_load(reinterpret_cast<const NV*>(qc + g * VEC));
                tv = *reinterpret_cast<Pack<T, VEC>*>(&a);
                qv = *reinterpret_cast<Pack<T, VEC>*>(&b);
            } else {
                tv.v[0] = at(tc, g);
                qv.v[0] = at(qc, g);
            }
#pragma unroll
            for (int e = VEC - 1; e >= 0; --e) {
                const int k = g * VEC + e;
                if (k < n) w.step(k, n, layer_thickness(A, B, k, sp, (double)tv.v[e], (double)qv.v[e]), tdphi);
            }
        }
    }
    const double ph_n = A[n] + B[n] * sp;  // p_half[n]
    double result;
    if (w.count == 0) {  // below the lowest full level: between the surface and that level
        result = ph_n + tdphi / w.bottom * (full_level(A, B, n - 1, sp) - ph_n);
    } else {
        int a, b;
        double da, db;
        if (w.count == n) {  // above the top full level: a = -1 wraps to the bottom level, b = 0
            a = n - 1;
            b = 0;
            da = w.bottom;
            db = w.dphi;
        } else {
            a = n - 1 - w.count;
            b = a + 1;
            if (a == w.a0) {
                da = w.da;
                db = w.db;
            } else {  // dphi is not monotone in this column: walk again, bottom to a
                double s = 0.0;
                da = db = 0.0;
                for (int k = n - 1; k >= a; --k) {
                    const int64_t i = LAYOUT == ATX_FIELDS ? (int64_t)k * pitch + p : p * pitch + k;
                    s = s + layer_thickness(A, B, k, sp, (double)t[i], (double)q[i]);
                    if (k == b) db = s;
                }
                da = s;
            }
        }
        const double fb = full_level(A, B, b, sp);
        result = fb + (tdphi - db) / (da - db) * (full_level(A, B, a, sp) - fb);
    }
    out[p] = (T)result;
}

template <typename T>
static int pressure_typed(const void* t, const void* q, const void* sp, const double* A, const double* B, int64_t n_pts, int n_lev,
                          int64_t pitch, int layout, double height, void* out, hipStream_t st) {
    const int64_t blocks = (n_pts + kBlock - 1) / kBlock;
    const double tdphi = height * kGravity;
    const T* tt = static_cast<const T*>(t);
    const T* qq = static_cast<const T*>(q);
    const T* ss = static_cast<const T*>(sp);
    T* oo = static_cast<T*>(out);
    constexpr int VEC = Vec16<T>::N;
    if (layout == ATX_FIELDS) {
        hipLaunchKernelGGL((pressure_at_height_kernel<T, ATX_FIELDS, 1>), dim3((unsigned)blocks), dim3(kBlock), 0, st, tt, qq, ss, A, B,
                           n_pts, n_lev, pitch, tdphi, oo);
    } else if (pitch % VEC == 0 && aligned16(t) && aligned16(q)) {
        hipLaunchKernelGGL((pressure_at_height_kernel<T, ATX_COLUMNS, VEC>), dim3((unsigned)blocks), dim3(kBlock), 0, st, tt, qq, ss, A,
                           B, n_pts, n_lev, pitch, tdphi, oo);
    } else {
        hipLaunchKernelGGL((pressure_at_height_kernel<T, ATX_COLUMNS, 1>), dim3((unsigned)blocks), dim3(kBlock), 0, st, tt, qq, ss, A, B,
                           n_pts, n_lev, pitch, tdphi, oo);
    }
    ATX_LAUNCH_CHECK("pressure_at_height_stack");
    return ATX_OK;
}

}  // namespace atx

using namespace atx;

extern "C" int atx_pressure_at_height_stack(const void* t, const void* q, const void* sp, const double* A, const double* B,
                                            int64_t n_pts, int64_t n_lev, int64_t pitch, int dtype, int layout, double height,
                                            void* out, void* stream) {
    ATX_REQUIRE((t && q && sp && out) || n_pts == 0, ATX_EINVAL, "atx_pressure_at_height_stack: null pointer");  // (an empty stack may have no storage)
    ATX_REQUIRE(A && B, ATX_EINVAL, "atx_pressure_at_height_stack: null A / B coefficients");
    ATX_REQUIRE(dtype == ATX_F32 || dtype == ATX_F64, ATX_EINVAL, "atx_pressure_at_height_stack: bad dtype %d", dtype);
    ATX_REQUIRE(layout == ATX_COLUMNS || layout == ATX_FIELDS, ATX_EINVAL, "atx_pressure_at_height_stack: bad layout %d", layout);
    ATX_REQUIRE(n_pts >= 0 && n_lev > 0 && n_lev < INT32_MAX, ATX_EINVAL, "atx_pressure_at_height_stack: bad sizes");
    ATX_REQUIRE(pitch >= (layout == ATX_COLUMNS ? n_lev : n_pts), ATX_ESHAPE, "atx_pressure_at_height_stack: pitch %lld too small",
                (long long)pitch);
    ATX_REQUIRE(n_pts / kBlock < 0x7fffffffll, ATX_EINVAL, "atx_pressure_at_height_stack: too many points");
    if (n_pts == 0) return ATX_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == ATX_F32) return pressure_typed<float>(t, q, sp, A, B, n_pts, (int)n_lev, pitch, layout, height, out, s);
    return pressure_typed<double>(t, q, sp, A, B, n_pts, (int)n_lev, pitch, layout, height, out, s);
}
