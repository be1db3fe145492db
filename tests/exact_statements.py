"""Exact (mpmath, 128-bit) restatements of the floating-point statements of the combine and exp / log kernels, an ulp measure against
them, and the input generators that tests/test_exact_statements.py (the reference's own arithmetic) and tests/test_gpu_ulp_budgets.py
(the kernels) share.

Every statement is evaluated on the EXACT input values, with every literal constant rounded to the stack's dtype first — what numpy
(NEP 50: a Python float next to a float32 array becomes a float32) and the kernels' ``T(c)`` both use.  Two kinds of reference:

- single-function operators (exp, log, cos / sin, atan2, hypot, snow_cover's tanh, polar_to_xy): the exact function of its argument AS
  THE STATEMENT'S OWN ARITHMETIC ROUNDS IT — the argument is rounded like numpy rounds it (``arguments_*`` below, which the CPU tests hold
  bit for bit against numpy's own intermediates), then everything after it is exact;
- composed statements (humidity, wind direction with its wrap): the whole statement, exact from the inputs.

A value of the reference is an ``mpmath.mpf`` (a finite, nonzero real) or a Python float: NaN, +-inf, or a zero whose sign the statement
defines — those have to be matched exactly.
"""

from __future__ import annotations

import json
import math
import os

import mpmath
import numpy as np

import vertical_restatement as vr

PREC = 128
mp = mpmath.mp
mp.prec = PREC

# the oracle's constants (oracle/oracle.py), as Python floats: numpy rounds them to the array's dtype
MET_C1, MET_T0, MET_TI = 611.21, 273.16, 273.16 - 23.0
MET_EPSILON = 287.0597 / 461.5250
RAD = math.pi / 180.0  # np.deg2rad's factor (float32 too: np.deg2rad(x) == x * float32(pi / 180), checked in the CPU tests)
DEG_POLAR = 180.0 / math.pi  # xy_to_polar's `* (180.0 / np.pi)`


def rad2deg_factor(dtype) -> float:
    """np.rad2deg's factor in ``dtype``: float32 uses 180f / pi_f (one ulp away from float32(180 / pi))."""
    return float(np.rad2deg(dtype(1.0)))


# ---- exact values ----------------------------------------------------------------------------------------------------------
def _fmt(dtype):
    """(precision in bits, frexp exponent of the smallest normal, frexp exponent just past the largest finite)."""
    return (53, -1021, 1024) if np.dtype(dtype) == np.float64 else (24, -125, 128)


def round_to(x, dtype):
    """``x`` (mpf) rounded to nearest-even in ``dtype``, subnormals and overflow included, as a Python float (+-inf on overflow)."""
    p, emin, emax = _fmt(dtype)
    if x == 0:
        return 0.0
    _, e = mpmath.frexp(x)
    q = mpmath.ldexp(1, max(e, emin) - p)
    r = mpmath.nint(x / q) * q
    if abs(r) >= mpmath.ldexp(1, emax):
        return math.copysign(math.inf, float(x))
    return float(r)


def ulp_of(r: float, dtype):
    """One ulp of the dtype value ``r``: 2^(exponent - precision + 1), the subnormal step below the normal range."""
    p, emin, _ = _fmt(dtype)
    e = math.frexp(r)[1] if r != 0 else emin
    return mpmath.ldexp(1, max(e, emin) - p)


def ulp_errors(got: np.ndarray, exact: np.ndarray, dtype) -> np.ndarray:
    """|got - exact| in ulps of the exact value rounded to ``dtype``.  Special references (Python floats: NaN, +-inf, signed zero) and
    exact values that overflow the dtype give 0 where ``got`` is that value bit for bit (any NaN for NaN) and inf where it is not;
    a non-finite ``got`` against a finite reference is inf as well."""
    got = np.asarray(got).reshape(-1)
    out = np.empty(got.size)
    for i, (g, x) in enumerate(zip(got.tolist(), exact.reshape(-1).tolist())):
        if isinstance(x, float):
            same = (math.isnan(g) and math.isnan(x)) or (g == x and math.copysign(1.0, g) == math.copysign(1.0, x))
            out[i] = 0.0 if same else math.inf
            continue
        r = round_to(x, dtype)
        if math.isinf(r):
            out[i] = 0.0 if g == r else math.inf
        elif not math.isfinite(g):
            out[i] = math.inf
        else:
            out[i] = float(abs(mpmath.mpf(g) - x) / ulp_of(r, dtype))
    return out


def _special(values) -> bool:
    return any(not math.isfinite(v) for v in values)


def _exact_array(fn, *arrays) -> np.ndarray:
    cols = [np.asarray(a).reshape(-1).tolist() for a in arrays]
    out = np.empty(len(cols[0]), dtype=object)
    for i, xs in enumerate(zip(*cols)):
        out[i] = fn(*xs)
    return out


# single-function operators -------------------------------------------------------------------------------------------------
def exp_exact(x: float):
    if math.isnan(x):
        return math.nan
    if math.isinf(x):
        return math.inf if x > 0 else 0.0
    return mpmath.exp(x)


def log_exact(x: float):
    if math.isnan(x) or x < 0:
        return math.nan
    if x == 0:
        return -math.inf
    if math.isinf(x):
        return math.inf
    if x == 1.0:
        return 0.0  # +0: IEEE log(1)
    return mpmath.log(x)


def cos_exact(a: float):
    """cos of the (already rounded) argument."""
    return math.nan if not math.isfinite(a) else mpmath.cos(a)


def sin_exact(a: float):
    if not math.isfinite(a):
        return math.nan
    return a if a == 0 else mpmath.sin(a)  # sin(+-0) = +-0


def atan2_exact(y: float, x: float):
    """IEEE atan2: the special operands (a zero, an infinity, NaN) give numpy's values — a signed zero, NaN, or an exact multiple of pi/4."""
    if _special((y, x)) or y == 0 or x == 0:
        r = float(np.arctan2(y, x))
        if r == 0 or math.isnan(r):
            return r
        return mpmath.pi / 4 * round(r / (math.pi / 4))
    return mpmath.atan2(y, x)


def hypot_exact(x: float, y: float):
    if math.isinf(x) or math.isinf(y):
        return math.inf
    if math.isnan(x) or math.isnan(y):
        return math.nan
    if x == 0 and y == 0:
        return 0.0
    return mpmath.sqrt(mpmath.mpf(x) ** 2 + mpmath.mpf(y) ** 2)


def tanh_exact(a: float):
    if math.isnan(a) or a == 0:
        return a
    return mpmath.tanh(a)


# the arguments as the statements round them (numpy, in the stack's dtype) ---------------------------------------------------
def argument_deg2rad(x: np.ndarray) -> np.ndarray:
    """np.deg2rad(x): fl(x * pi/180)."""
    return x * x.dtype.type(RAD)


def argument_polar(direction: np.ndarray) -> np.ndarray:
    """polar_to_xy's a = fl(fl(270 - direction) * pi/180)."""
    dt = direction.dtype.type
    return (dt(270.0) - direction) * dt(RAD)


def argument_snow_cover(sd: np.ndarray, rsn: np.ndarray) -> np.ndarray:
    """snow_cover's tanh argument fl(fl(4000 * fl(fl(1000 * sd) / rsn)) / clip(rsn, 100, 400))."""
    dt = sd.dtype.type
    with np.errstate(all="ignore"):
        return (dt(4000) * ((dt(1000) * sd) / rsn)) / np.clip(rsn, dt(100), dt(400))


def polar_u_exact(speed: float, a: float):
    """speed * cos(a) exact, a rounded."""
    if _special((speed, a)):
        return float(np.float64(speed) * np.cos(np.float64(a)))
    return speed * mpmath.cos(a) if speed != 0 else float(np.float64(speed) * np.cos(a))


def polar_v_exact(speed: float, a: float):
    if _special((speed, a)) or speed == 0 or a == 0:
        return float(np.float64(speed) * np.sin(np.float64(a)))
    return speed * mpmath.sin(a)


# composed statements ---------------------------------------------------------------------------------------------------------
class Consts:
    """The statements' literal constants rounded to ``dtype`` (a Python float expression is evaluated in float64 first, as Python does)."""

    def __init__(self, dtype):
        c = lambda v: mpmath.mpf(float(np.dtype(dtype).type(v)))  # noqa: E731
        self.c1, self.t0, self.ti = c(MET_C1), c(MET_T0), c(MET_TI)
        self.inv_range = c(1.0 / (MET_T0 - MET_TI))
        self.aw, self.bw, self.ai, self.bi = c(17.502), c(32.19), c(22.587), c(-0.7)
        self.eps, self.k = c(MET_EPSILON), c(MET_EPSILON * (1.0 / MET_EPSILON - 1.0))
        self.one_m_eps, self.guard, self.rzero = c(1.0 - MET_EPSILON), c(1.0e-4), c(1.0e-4)
        self.qzero = c(1.0e-8)
        self.dp_num = c(17.502 * MET_T0)
        self.deg_polar, self.rad2deg = c(DEG_POLAR), c(rad2deg_factor(np.dtype(dtype).type))


def _es_water(k: Consts, t):
    return k.c1 * mpmath.exp(k.aw * (t - k.t0) / (t - k.bw))


def _es_ice(k: Consts, t):
    return k.c1 * mpmath.exp(k.ai * (t - k.t0) / (t - k.bi))


def _es_mixed(k: Consts, t):
    alpha = min(mpmath.mpf(1), (max(k.ti, min(k.t0, t)) - k.ti) * k.inv_range) ** 2
    ew = _es_water(k, t) if alpha > 0 else 0
    ei = _es_ice(k, t) if alpha < 1 else 0
    return alpha * ew + (1 - alpha) * ei


def r_to_d_exact(k: Consts, r: float, t: float):
    """dewpoint_from_relative_humidity: r == 0 -> 1e-4 (rounded), ln = log(r es_water(t) / 100 / c1), (32.19 ln - c(17.502 T0)) / (ln - 17.502)."""
    if _special((r, t)):
        return math.nan
    r = k.rzero if r == 0 else mpmath.mpf(r)
    ln = mpmath.log(r * _es_water(k, t) / 100 / k.c1)
    return (k.bw * ln - k.dp_num) / (ln - k.aw)


def d_to_r_exact(k: Consts, td: float, t: float):
    """relative_humidity_from_dewpoint: 100 es_water(td) / es_water(t)."""
    if _special((td, t)):
        return math.nan
    return 100 * _es_water(k, td) / _es_water(k, t)


def q_to_r_exact(k: Consts, q: float, t: float, p: float):
    """relative_humidity_from_specific_humidity: e = p q / (eps + c(eps (1/eps - 1)) q), 100 e / es_mixed(t)."""
    if _special((q, t, p)):
        return math.nan
    e = mpmath.mpf(p) * q / (k.eps + k.k * q)
    return 100 * e / _es_mixed(k, t)


def r_to_q_exact(k: Consts, r: float, t: float, p: float, guarded: bool = True):
    """specific_humidity_from_relative_humidity: e = r es_mixed(t) / 100; NaN where p - e < 1e-4; eps e / (p - c(1 - eps) e)."""
    if _special((r, t, p)):
        return math.nan
    e = mpmath.mpf(r) * _es_mixed(k, t) / 100
    if guarded and p - e < k.guard:
        return math.nan
    return k.eps * e / (p - k.one_m_eps * e)


GUARD_BAND_ULPS = 256


def in_guard_band(k: Consts, r, t, p, dtype) -> np.ndarray:
    """Where |p - e - 1e-4| (exact) is within GUARD_BAND_ULPS ulps of p: there numpy's e — tens of ulps from the exact one — and the
    kernel's may decide the guard of specific_humidity_from_vapour_pressure either way, and both sides are the statement's own value."""
    eps = float(np.finfo(dtype).eps)
    out = np.zeros(len(r), dtype=bool)
    for i, (ri, ti, pi) in enumerate(zip(np.asarray(r, float), np.asarray(t, float), np.asarray(p, float))):
        if math.isfinite(ri + ti + pi):
            e = mpmath.mpf(ri) * _es_mixed(k, ti) / 100
            out[i] = abs(pi - e - k.guard) <= GUARD_BAND_ULPS * eps * abs(pi)
    return out


def q_to_d_exact(k: Consts, q: float, p: float):
    """dewpoint_from_specific_humidity (tests/vertical_restatement.py): q == 0 -> 1e-8 (rounded), e = p q / (eps + c(eps (1/eps - 1)) q),
    ln = log(e / c1), (32.19 ln - c(17.502 T0)) / (ln - 17.502)."""
    if _special((q, p)):
        return math.nan
    q = k.qzero if q == 0 else mpmath.mpf(q)
    e = mpmath.mpf(p) * q / (k.eps + k.k * q)
    if e <= 0:
        return math.nan
    ln = mpmath.log(e / k.c1)
    return (k.bw * ln - k.dp_num) / (ln - k.aw)


def d_to_q_exact(k: Consts, td: float, p: float, guarded: bool = True):
    """specific_humidity_from_dewpoint: e = es_water(td); NaN where p - e < 1e-4; eps e / (p - c(1 - eps) e).  Non-finite operands give
    what numpy's statement gives."""
    if _special((td, p)):
        with np.errstate(all="ignore"):
            return float(vr.specific_humidity_from_dewpoint(np.array([td]), np.array([p]))[0])
    e = _es_water(k, mpmath.mpf(td))
    if guarded and p - e < k.guard:
        return math.nan
    return k.eps * e / (p - k.one_m_eps * e)


def in_guard_band_d(k: Consts, td, p, dtype) -> np.ndarray:
    """``in_guard_band`` for specific_humidity_from_dewpoint: e = es_water(td)."""
    eps = float(np.finfo(dtype).eps)
    out = np.zeros(len(td), dtype=bool)
    for i, (ti, pi) in enumerate(zip(np.asarray(td, float), np.asarray(p, float))):
        if math.isfinite(ti + pi):
            out[i] = abs(pi - _es_water(k, mpmath.mpf(ti)) - k.guard) <= GUARD_BAND_ULPS * eps * abs(pi)
    return out


def direction_deg_exact(k: Consts, s: float, c: float):
    """direction_from_cos_sin(degrees=True): rad2deg(atan2(s, c)) with the wrap to [0, 360), exact."""
    a = atan2_exact(s, c)
    if isinstance(a, float):
        return a  # NaN, or a signed zero, which neither the product nor the wrap changes
    d = a * k.rad2deg
    d = d - 360 if d >= 360 else d
    d = d + 360 if d < 0 else d
    return d if d != 0 else 0.0


def polar_direction_exact(k: Consts, u: float, v: float):
    """xy_to_polar's direction: mod(270 - atan2(v, u) * c(180 / pi), 360), exact."""
    a = atan2_exact(v, u)
    if isinstance(a, float):
        if math.isnan(a):
            return a
        a = mpmath.mpf(a)
    d = 270 - a * k.deg_polar
    d = d - 360 if d >= 360 else d
    return d if d != 0 else 0.0


def consts(dtype) -> Consts:
    return Consts(dtype)


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def ladder(centre, dtype, half: int = 64) -> np.ndarray:
    """The 2 * half + 1 representable numbers around dtype(centre), one ulp apart (positive centre)."""
    bits = np.int32 if np.dtype(dtype) == np.float32 else np.int64
    c = np.array([centre], dtype=dtype).view(bits)[0]
    return (c + np.arange(-half, half + 1).astype(bits)).view(dtype)


def near_multiples(base: float, count: int, dtype, rng, steps: int = 3) -> np.ndarray:
    """Values within ``steps`` ulps of the dtype's nearest value to m * base, for m in [-count, count]."""
    m = np.arange(-count, count + 1, dtype=np.float64)
    centre = (m * base).astype(dtype)
    out = [centre]
    for s in range(1, steps + 1):
        up, down = centre.copy(), centre.copy()
        for _ in range(s):
            up, down = np.nextafter(up, dtype(np.inf)), np.nextafter(down, dtype(-np.inf))
        out += [up, down]
    return np.concatenate(out)


def _cases(dtype, parts):
    """{case name: tuple of arrays} in ``dtype``."""
    return {name: tuple(np.asarray(a, dtype=dtype) for a in arrays) for name, arrays in parts.items()}


def humidity_cases(kind: str, dtype, n: int = 4096, seed: int = 0) -> dict:
    """Inputs of one humidity statement: ``kind`` in r_to_d (r, t), d_to_r (td, t), q_to_r (q, t, p), r_to_q (r, t, p), q_to_d (q, p),
    d_to_q (td, p)."""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype).type
    t = lambda m: rng.uniform(150.0, 350.0, m)  # noqa: E731
    lad = np.concatenate([ladder(MET_TI, dtype), ladder(MET_T0, dtype)])  # the mixed phase's ends, 64 ulps either side
    p = lambda m: 10.0 ** rng.uniform(2.0, math.log10(1.1e5), m)  # noqa: E731
    sub_lo, sub_hi = (2.0**-1023, 2.0**-1022) if dt is np.float64 else (2.0**-127, 2.0**-126)  # the top binade of the subnormals
    if kind in ("r_to_d", "d_to_r"):
        if kind == "r_to_d":
            parts = {
                "atmosphere": (rng.uniform(0.5, 110.0, n), t(n)),
                "r = 0 and above 100": (np.where(np.arange(n // 4) % 2 == 0, 0.0, rng.uniform(100.0, 150.0, n // 4)), t(n // 4)),
                "subnormal r": (rng.uniform(sub_lo, sub_hi, n // 8), rng.uniform(250.0, 320.0, n // 8)),
                "mixed-phase ends": (rng.uniform(1.0, 100.0, lad.size), lad),
            }
        else:
            tt = t(n)
            parts = {
                "atmosphere": (tt - rng.uniform(0.0, 40.0, n), tt),
                "mixed-phase ends": (lad - rng.uniform(0.0, 5.0, lad.size), lad),
            }
        return _cases(dtype, {**parts, "specials": _humidity_specials(kind, dtype)})
    if kind == "q_to_r":
        parts = {
            "atmosphere": (10.0 ** rng.uniform(-8.0, math.log10(0.05), n), t(n), p(n)),
            "mixed-phase ends": (10.0 ** rng.uniform(-6.0, -2.0, lad.size), lad, rng.uniform(5e4, 1.05e5, lad.size)),
        }
        return _cases(dtype, {**parts, "specials": _humidity_specials(kind, dtype)})
    if kind == "q_to_d":
        zeros = np.where(np.arange(n // 4) % 2 == 0, 0.0, rng.uniform(sub_lo, sub_hi, n // 4))
        parts = {
            "atmosphere": (10.0 ** rng.uniform(-8.0, math.log10(0.05), n), p(n)),
            "q = 0 and subnormal": (zeros, p(n // 4)),
        }
        return _cases(dtype, {**parts, "specials": _humidity_specials(kind, dtype)})
    if kind == "d_to_q":
        # the guard band: p within 48 ulps of es_water(td) + 1e-4
        k = consts(dtype)
        tb = rng.uniform(280.0, 320.0, n // 8).astype(dtype)
        e = np.array([float(_es_water(k, mpmath.mpf(float(tt)))) for tt in tb])
        bits = np.int32 if dt is np.float32 else np.int64
        pb = ((e + 1.0e-4).astype(dtype).view(bits) + rng.integers(-48, 49, e.size).astype(bits)).view(dtype)
        parts = {
            "atmosphere": (t(n), p(n)),  # es_water(350 K) = 41 kPa: the guard's NaN occurs
            "guard band": (tb, pb),
        }
        return _cases(dtype, {**parts, "specials": _humidity_specials(kind, dtype)})
    assert kind == "r_to_q"
    # the guard band: p - e within a few parts in 1e6 of 1e-4 (e = r es_mixed(t) / 100 chosen to hit it)
    k = consts(dtype)
    tb = rng.uniform(280.0, 320.0, n // 8)
    rb = rng.uniform(50.0, 100.0, n // 8).astype(dtype)
    tb = tb.astype(dtype)
    e = np.array([float(mpmath.mpf(float(r)) * _es_mixed(k, float(tt)) / 100) for r, tt in zip(rb, tb)])
    bits = np.int32 if dt is np.float32 else np.int64
    pb = ((e + 1.0e-4).astype(dtype).view(bits) + rng.integers(-48, 49, e.size).astype(bits)).view(dtype)  # within 48 ulps of p = e + 1e-4
    parts = {
        "atmosphere": (rng.uniform(0.5, 110.0, n), t(n), p(n)),
        "mixed-phase ends": (rng.uniform(1.0, 100.0, lad.size), lad, rng.uniform(5e4, 1.05e5, lad.size)),
        "guard band": (rb, tb, pb),
    }
    parts["specials"] = _humidity_specials(kind, dtype)
    return _cases(dtype, parts)


def _humidity_specials(kind: str, dtype) -> tuple:
    """NaN and +-inf in every operand but the pressure (an infinite pressure makes numpy's q_to_r infinite, not NaN): NaN results."""
    s = [np.nan, np.inf, -np.inf]
    ok = {"r_to_d": 50.0, "d_to_r": 280.0, "q_to_r": 0.01, "r_to_q": 50.0, "q_to_d": 0.01, "d_to_q": 280.0}[kind]
    x = np.array(s + [ok] * 3)
    if kind in ("q_to_d", "d_to_q"):  # (x, p): the pressure is the second operand — NaN only: an infinite pressure is an infinite divisor,
        # outside the domain of the kernels' `quotient` (csrc/atx_combine.hip), as for q_to_r above
        return (x, np.array([85000.0] * 3 + [np.nan, 85000.0, 85000.0]))
    t = np.array([280.0] * 3 + s)
    return (x, t) if kind in ("r_to_d", "d_to_r") else (x, t, np.full(6, 85000.0))


def level_pressures(dtype, n_lev: int, seed: int = 0) -> np.ndarray:
    """Levels in hPa for the two-operand humidity forms (p = fl(100 * level))."""
    rng = np.random.default_rng(seed)
    return np.sort(rng.uniform(1.0, 1100.0, n_lev))


def sincos_cases(dtype, degrees: bool, n: int = 4096, seed: int = 1) -> dict:
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype).type
    if degrees:
        parts = {
            "[-720, 720]": (rng.uniform(-720.0, 720.0, n),),
            "near 0, 90 ... 360": (near_multiples(90.0, 4, dtype, rng, steps=8),),
            "tiny": (np.concatenate([10.0 ** rng.uniform(-40 if dt is np.float32 else -300, -5, n // 8), [0.0, -0.0]]),),
        }
    else:
        big = 1.0e30 if dt is np.float32 else 1.0e300
        parts = {
            "[-2 pi, 2 pi]": (rng.uniform(-2 * math.pi, 2 * math.pi, n),),
            "[-1e5, 1e5]": (rng.uniform(-1.0e5, 1.0e5, n),),
            "beyond 1e5": (np.concatenate([10.0 ** rng.uniform(5.0, math.log10(big), n // 4), -(10.0 ** rng.uniform(5.0, 8.0, n // 8))]),),
            "next to multiples of pi/2": (near_multiples(math.pi / 2, 200, dtype, rng, steps=3),),
            "tiny": (np.concatenate([10.0 ** rng.uniform(-40 if dt is np.float32 else -300, -3, n // 8), -(10.0 ** rng.uniform(-30, -3, n // 8))]),),
        }
    return _cases(dtype, parts)


def atan2_cases(dtype, n: int = 4096, seed: int = 2) -> dict:
    """(y, x) pairs: the sin / cos operands of direction_from_cos_sin and the (v, u) of xy_to_polar (the test maps them)."""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype).type
    fin = np.finfo(dtype)
    ang = rng.uniform(-math.pi, math.pi, n)
    r = rng.uniform(0.1, 30.0, n)
    eps_side = 10.0 ** rng.uniform(-30 if dt is np.float32 else -300, -1, n // 4)
    signs = rng.choice([-1.0, 1.0], n // 4)
    mag = rng.uniform(0.5, 20.0, n // 4) * rng.choice([-1.0, 1.0], n // 4)
    d = rng.uniform(0.5, 20.0, n // 8)
    diag = d * (1.0 + rng.uniform(-1e-6, 1e-6, n // 8))
    big = 10.0 ** rng.uniform(math.log10(float(fin.max)) - 6, math.log10(float(fin.max)) - 0.01, n // 8)
    tiny = 10.0 ** rng.uniform(math.log10(float(fin.smallest_subnormal)) + 1, math.log10(float(fin.tiny)) + 2, n // 8)
    far = 10.0 ** rng.uniform(-20, 20, (2, n // 8))
    # direction near the 0 / 360 wrap: tiny negative and positive angles with a positive x (and the same for v, u of the wind: u < 0)
    wrap = rng.choice([-1.0, 1.0], n // 8) * 10.0 ** rng.uniform(-12 if dt is np.float32 else -30, -2, n // 8)
    parts = {
        "circle": (r * np.sin(ang), r * np.cos(ang)),
        "next to the axes": (
            np.concatenate([eps_side * signs, mag]),
            np.concatenate([mag, eps_side * signs]),
        ),
        "diagonals": (np.concatenate([diag, -diag, diag, -diag]), np.concatenate([d, d, -d, -d])),
        "enormous": (big * rng.choice([-1.0, 1.0], big.size), big[::-1] * rng.choice([-1.0, 1.0], big.size)),
        "minute": (tiny * rng.choice([-1.0, 1.0], tiny.size), tiny[::-1] * rng.choice([-1.0, 1.0], tiny.size)),
        "far apart": (far[0] * rng.choice([-1.0, 1.0], far.shape[1]), far[1] * rng.choice([-1.0, 1.0], far.shape[1])),
        "near the wrap": (np.concatenate([wrap, wrap]), np.concatenate([np.ones(wrap.size), -np.ones(wrap.size)])),
    }
    return _cases(dtype, parts)


def special_pairs(dtype):
    """Every pairing of 0, -0, 1, -1, +-inf, NaN and a subnormal: the IEEE special cases of two-operand statements."""
    v = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, float(np.finfo(dtype).smallest_subnormal), 3.5], dtype=dtype)
    a, b = np.meshgrid(v, v)
    return a.reshape(-1), b.reshape(-1)


def exp_cases(dtype, n: int = 4096, seed: int = 3) -> dict:
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype).type
    over = float(np.log(np.finfo(dtype).max))  # 709.78 / 88.72
    under = math.log(float(np.finfo(dtype).smallest_subnormal))  # -744.4 / -103.3
    tiny_edge = math.log(float(np.finfo(dtype).tiny))  # -708.4 / -87.3
    parts = {
        "surface pressure logs": (rng.uniform(9.0, 12.0, n),),
        "whole range": (rng.uniform(under - 5, over + 5, n),),
        "overflow threshold": (ladder(over, dtype, 256),),
        "subnormal results": (rng.uniform(under, tiny_edge, n // 2),),
        "near 0": (np.concatenate([rng.uniform(-1e-3, 1e-3, n // 4), 10.0 ** rng.uniform(-40 if dt is np.float32 else -300, -8, n // 8), [0.0, -0.0]]),),
        "specials": (np.array([np.inf, -np.inf, np.nan, 1e30, -1e30, over, -over]),),
    }
    return _cases(dtype, parts)


def log_cases(dtype, n: int = 4096, seed: int = 4) -> dict:
    rng = np.random.default_rng(seed)
    fin = np.finfo(dtype)
    parts = {
        "surface pressure (Pa)": (rng.uniform(3.0e4, 1.1e5, n),),
        "every magnitude": (10.0 ** rng.uniform(math.log10(float(fin.tiny)), math.log10(float(fin.max)) - 0.01, n),),
        "near 1": (np.concatenate([1.0 + rng.uniform(-1e-3, 1e-3, n // 2), ladder(1.0, dtype, 256)]),),
        "subnormal": (rng.uniform(float(fin.smallest_subnormal), float(fin.tiny), n // 2),),
        "specials": (np.array([0.0, -0.0, -1.0, -np.inf, np.inf, np.nan, 1.0, float(fin.max), float(fin.smallest_subnormal)]),),
    }
    return _cases(dtype, parts)


def snow_cases(dtype, n: int = 4096, seed: int = 5) -> dict:
    rng = np.random.default_rng(seed)
    rsn = rng.uniform(50.0, 600.0, n)
    # depths spread over the tanh's whole working range (argument 1e-8 .. 3): sd = arg * rsn * clip(rsn) / 4e6
    arg = 10.0 ** rng.uniform(-8.0, math.log10(3.0), n)
    parts = {
        "tanh range": (arg * rsn * np.clip(rsn, 100, 400) / 4.0e6, rsn),
        "random depths": (rng.uniform(0.0, 0.3, n // 4), rng.uniform(50.0, 600.0, n // 4)),
        "zero and negative depths": (np.array([0.0, -0.0, -1e-3, -0.5, 1e-3]), np.array([200.0, 200.0, 200.0, 50.0, 700.0])),
    }
    return _cases(dtype, parts)


def wind_cases(dtype, n: int = 4096, seed: int = 6) -> dict:
    """(u, v) for xy_to_polar; (speed, direction) for polar_to_xy come from them."""
    rng = np.random.default_rng(seed)
    return _cases(dtype, {"wind": (rng.normal(0.0, 8.0, n), rng.normal(0.0, 8.0, n))})


def polar_cases(dtype, n: int = 4096, seed: int = 7) -> dict:
    """(speed, direction in degrees), directions next to multiples of 90 included (the argument of cos / sin next to multiples of pi/2)."""
    rng = np.random.default_rng(seed)
    near = near_multiples(90.0, 4, dtype, rng, steps=8)
    near = near[(near >= 0) & (near < 360)]
    return _cases(dtype, {
        "directions": (rng.uniform(0.0, 40.0, n), rng.uniform(0.0, 360.0, n)),
        "next to the axes": (rng.uniform(0.1, 40.0, near.size), near),
    })


def w_cases(dtype, n: int = 4096, seed: int = 8):
    """(w, t, q) and levels in hPa for w_to_wz / wz_to_w, with NaN, +-inf, +-0 and subnormal vertical velocities."""
    rng = np.random.default_rng(seed)
    w = rng.normal(0.0, 0.5, n)
    fin = np.finfo(dtype)
    w[:8] = [0.0, -0.0, np.inf, -np.inf, np.nan, float(fin.smallest_subnormal), -float(fin.tiny) / 3, float(fin.max)]
    t = rng.uniform(180.0, 320.0, n)
    t[8:10] = [np.nan, np.inf]
    q = rng.uniform(0.0, 0.03, n)
    q[10:12] = [-0.0, float(fin.smallest_subnormal)]
    return tuple(np.asarray(a, dtype=dtype) for a in (w, t, q))


def arithmetic_cases(dtype, n: int = 4096, seed: int = 9):
    """Operands of the one-rounding operators (SNOW_DEPTH_M, SUB, SUM): ordinary values and every special one."""
    rng = np.random.default_rng(seed)
    fin = np.finfo(dtype)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, float(fin.smallest_subnormal), -float(fin.smallest_subnormal),
                        float(fin.tiny), float(fin.max), -float(fin.max), 1.0, -1.0])
    cols = []
    for k in range(4):
        c = rng.normal(0.0, 100.0, n) * 10.0 ** rng.uniform(-3, 3, n)
        c[: special.size * special.size] = np.tile(special, special.size) if k % 2 == 0 else np.repeat(special, special.size)
        c[special.size**2 : special.size**2 + 64] = rng.uniform(-1, 1, 64) * float(fin.tiny)  # subnormal sums and differences
        cols.append(c.astype(dtype))
    return cols


def exact_values(fn, *arrays) -> np.ndarray:
    """``fn`` over the elements (Python floats) of the arrays: an object array of mpf / float."""
    return _exact_array(fn, *arrays)


# ---- the statements, as both test files see them -------------------------------------------------------------------------------
N_LEV = 4  # every case is laid out as a stack of N_LEV levels (the two-operand humidity forms take their pressure from the level)
SINGLE, COMPOSED, DIRECTION, DEGREES = "single", "composed", "direction", "degrees"


class Statement:
    """One operator's inputs (``[N_LEV, n]`` arrays, in the stack's dtype), per output: the exact reference (object array, flat), numpy's
    value of the statement, which kind of reference it is; ``case`` names the generator of every point; ``alt`` maps an output to
    (mask, value): where the mask is set, ``value`` (NaN: the r_to_q guard; 1.0: the snow-cover jump) is the statement's own too."""

    def __init__(self, name, dtype, inputs, case, exact, numpy_out, kinds, levels=None, alt=None):
        self.name, self.dtype, self.inputs, self.case = name, np.dtype(dtype).type, inputs, case
        self.exact, self.numpy_out, self.kinds, self.levels, self.alt = exact, numpy_out, kinds, levels, alt or {}

    def errors(self, out: int, got: np.ndarray) -> np.ndarray:
        """Per point: ulps from the exact value — DIRECTION outputs within a degree of the 0 / 360 wrap, and DEGREES outputs everywhere,
        the circular distance in ulps of 360 instead (xy_to_polar rounds `270 - d` in [90, 450] before it takes 360 off: the relative
        error of what comes out of that subtraction means nothing); 0 where an ``alt`` value is met; inf where a
        special value is not matched."""
        got = np.asarray(got).reshape(-1)
        err = ulp_errors(got, self.exact[out], self.dtype)
        if self.kinds[out] in (DIRECTION, DEGREES):
            ulp360 = float(np.spacing(self.dtype(360.0)))
            for i, x in enumerate(self.exact[out].tolist()):
                wrap = self.kinds[out] == DEGREES or x < 1 or x > 359
                if not isinstance(x, float) and wrap and math.isfinite(got[i]):
                    d = abs(float(got[i]) - float(x)) % 360.0
                    err[i] = min(d, 360.0 - d) / ulp360
        if out in self.alt:
            mask, value = self.alt[out]
            hit = mask & ((np.isnan(got) & np.isnan(value)) | (got == value))
            err[hit] = 0.0
        return err

    def numpy_errors(self, out: int) -> np.ndarray:
        key = ("_np_err", out)
        if key not in self.__dict__:
            self.__dict__[key] = self.errors(out, self.numpy_out[out])
        return self.__dict__[key]


def _layout(parts: dict):
    """Concatenate the generators' arrays (repeated to a multiple of N_LEV) into [N_LEV, n] stacks, and the case name of every point."""
    names = [np.full(len(arrays[0]), name, dtype=object) for name, arrays in parts.items()]
    cols = [np.concatenate([arrays[i] for arrays in parts.values()]) for i in range(len(next(iter(parts.values()))))]
    names = np.concatenate(names)
    n = -(-names.size // N_LEV) * N_LEV
    return [np.resize(c, n).reshape(N_LEV, -1) for c in cols], np.resize(names, n).reshape(N_LEV, -1)


def _flat(*arrays):
    return [np.asarray(a).reshape(-1) for a in arrays]


_CACHE: dict = {}


def statement(name: str, dtype) -> Statement:
    """The Statement ``name`` in ``dtype`` — built once per process (the exact values take a few seconds at 128 bits)."""
    key = (name, np.dtype(dtype).name)
    if key not in _CACHE:
        _CACHE[key] = _build(name, np.dtype(dtype).type)
    return _CACHE[key]


def _build(name, dt) -> Statement:
    from oracle import oracle

    k = consts(dt)
    ex = exact_values
    with np.errstate(all="ignore"):
        if name in ("exp", "log"):
            (x,), case = _layout(exp_cases(dt) if name == "exp" else log_cases(dt))
            want = np.exp(x) if name == "exp" else np.log(x)
            return Statement(name, dt, [x], case, [ex(exp_exact if name == "exp" else log_exact, *_flat(x))], [want], [SINGLE])
        if name in ("cos_sin", "cos_sin_deg"):
            deg = name == "cos_sin_deg"
            (x,), case = _layout(sincos_cases(dt, deg))
            a = argument_deg2rad(x) if deg else x
            wc, ws = oracle.cos_sin(x, deg)
            return Statement(name, dt, [x], case, [ex(cos_exact, *_flat(a)), ex(sin_exact, *_flat(a))], [wc, ws], [SINGLE, SINGLE])
        if name in ("atan2", "atan2_deg"):
            parts = atan2_cases(dt)
            parts["specials"] = special_pairs(dt)
            (s, c), case = _layout(parts)
            want = oracle.direction_from_cos_sin(c, s, name == "atan2_deg")
            fn = atan2_exact if name == "atan2" else (lambda y, x: direction_deg_exact(k, y, x))
            return Statement(name, dt, [c, s], case, [ex(fn, *_flat(s, c))], [want], [SINGLE if name == "atan2" else DIRECTION])
        if name == "xy_to_polar":
            parts = atan2_cases(dt)
            parts["specials"] = special_pairs(dt)
            parts.update(wind_cases(dt))
            (v, u), case = _layout(parts)
            ws, wd = oracle.xy_to_polar(u, v)
            exact = [ex(hypot_exact, *_flat(u, v)), ex(lambda a, b: polar_direction_exact(k, a, b), *_flat(u, v))]
            return Statement(name, dt, [u, v], case, exact, [ws, wd], [SINGLE, DEGREES])
        if name == "polar_to_xy":
            (sp, d), case = _layout(polar_cases(dt))
            a = argument_polar(d)
            wu, wv = oracle.polar_to_xy(sp, d)
            return Statement(name, dt, [sp, d], case, [ex(polar_u_exact, *_flat(sp, a)), ex(polar_v_exact, *_flat(sp, a))], [wu, wv], [SINGLE, SINGLE])
        if name == "snow_cover":
            (sd, rsn), case = _layout(snow_cases(dt))
            arg = argument_snow_cover(sd, rsn)
            before = np.clip(np.tanh(arg), 0, 1)  # the statement before its jump
            exact = ex(lambda a, b: tanh_exact(a) if a > 0 else b, *_flat(arg, before))
            band = 8 * float(np.finfo(dt).eps)
            over = np.array([not isinstance(x, float) and x > 0.99 + band for x in exact.tolist()])
            exact[over] = 1.0  # beyond the jump the statement's value is 1.0, bit for bit
            near = np.array([not isinstance(x, float) and abs(x - 0.99) <= band for x in exact.tolist()])
            return Statement(name, dt, [sd, rsn], case, [exact], [oracle.snow_cover(sd, rsn)], [SINGLE], alt={0: (near, 1.0)})
        # humidity
        kind = name.removesuffix("_level")
        parts = humidity_cases(kind, dt)
        levels = None
        if name.endswith("_level"):  # (x, t) and p = fl(100 * level) from the level
            parts = {c: arrays[:2] for c, arrays in parts.items() if c != "guard band"}
            ins, case = _layout(parts)
            levels = level_pressures(dt, N_LEV)
            p = np.broadcast_to((dt(100.0) * levels.astype(dt))[:, None], ins[0].shape).astype(dt)
        else:
            ins, case = _layout(parts)
            p = ins[2] if len(ins) > 2 else None
        alt = {}
        if kind == "r_to_d":
            want, fn = oracle.dewpoint_from_relative_humidity(*ins), r_to_d_exact
        elif kind == "d_to_r":
            want, fn = oracle.relative_humidity_from_dewpoint(*ins), d_to_r_exact
        elif kind == "q_to_r":
            want, fn = oracle.relative_humidity_from_specific_humidity(ins[1], ins[0], p), q_to_r_exact
        elif kind == "q_to_d":
            want, fn = vr.dewpoint_from_specific_humidity(*ins), q_to_d_exact
        elif kind == "d_to_q":
            want, fn = vr.specific_humidity_from_dewpoint(*ins), d_to_q_exact
            band = in_guard_band_d(k, *_flat(*ins), dt)
            alt = {0: (band, np.nan)}
        else:
            want, fn = oracle.specific_humidity_from_relative_humidity(ins[1], ins[0], p), r_to_q_exact
            band = in_guard_band(k, *_flat(ins[0], ins[1], p), dt)
            alt = {0: (band, np.nan)}
        args = _flat(*ins[:2]) + ([p.reshape(-1)] if p is not None else [])
        exact = ex(lambda *a: fn(k, *a), *args)
        if kind in ("r_to_q", "d_to_q"):  # within the guard band the reference is the unguarded statement, and NaN is accepted too
            unguarded = r_to_q_exact if kind == "r_to_q" else d_to_q_exact
            exact[band] = ex(lambda *a: unguarded(k, *a, guarded=False), *[x[band] for x in args])
        return Statement(name, dt, ins, case, [exact], [want.astype(dt, copy=False)], [COMPOSED], levels=levels, alt=alt)


SINGLE_FUNCTION = ("exp", "log", "cos_sin", "cos_sin_deg", "atan2", "snow_cover", "polar_to_xy")
COMPOSED_STATEMENTS = ("atan2_deg", "xy_to_polar", "r_to_d", "d_to_r", "q_to_r", "r_to_q", "q_to_r_level", "r_to_q_level",
                       "q_to_d", "d_to_q")
ALL = SINGLE_FUNCTION + COMPOSED_STATEMENTS


# ---- the column statement: pressure_at_height_levels (tests/vertical_restatement.py, csrc/atx_vertical.hip) ---------------------
# Evaluated per column on the exact values of the stored numbers (float32 inputs widened exactly; A, B float64), with the constants as
# the float64 literals the statement uses: Rd, Rv, g, and alpha[0] = fl64(log 2) (numpy's np.log(2.0), the kernel's kLn2) — that double,
# not the exact ln 2.  tdphi = fl64(height * g) is rounded BEFORE the comparison, as numpy and the kernel's host side both do.
#
# No "either side" band is needed where tdphi meets a dphi[k]: the statement is continuous across every one of its branch boundaries —
# `below` meets `above` at p_full[n-1] (tdphi = dphi[n-1]), adjacent segments meet at p_full[k] (tdphi = dphi[k]), and the wrap of
# i == n (a = n-1, b = 0) meets the top segment at p_full[0] — so a count that the exact dphi and numpy's rounded one decide differently
# moves the value by no more than the slope times the rounding (tests/test_exact_statements.py checks the continuity).
#
# A level whose term cannot be evaluated (a NaN or an infinity in t or q, a half-level pressure ratio that is not positive, a zero
# layer thickness in pressure) makes dphi non-finite from that level to the top in numpy; the exact dphi is "special" there.  The count
# takes numpy's verdict at those levels (a NaN never counts, -inf always does); a result that needs a special dphi, a zero denominator
# (da == db: n_lev == 1 above the level; dphi[n-1] == 0) or a non-finite surface pressure is the value numpy's restatement gives — NaN
# or +-inf, matched as `ulp_errors` matches specials.
LN2_F64 = float(np.log(2.0))
_GOLDEN_AB = None


def hybrid_column(n):
    """n + 1 half levels of a hybrid column: pure pressure (A) near the top, terrain-following (B) near the ground, A[0] = B[0] = 0."""
    global _GOLDEN_AB
    if n == 2:  # the reference's own bottom levels, the top half level not at 0
        if _GOLDEN_AB is None:
            path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "height_level_humidity.json")
            _GOLDEN_AB = json.load(open(path))["AB"]
        return np.array(_GOLDEN_AB["A"]), np.array(_GOLDEN_AB["B"])
    eta = np.concatenate([[0.0], np.geomspace(2e-4, 1.0, n)]) if n > 1 else np.array([0.0, 1.0])
    B = np.clip((eta - 0.2) / 0.8, 0.0, 1.0) ** 1.5
    return 101325.0 * (eta - B) * 0.9, B


class ColumnProfile:
    """One column, exact: p_half, p_full (mpf lists) and dphi (mpf, or None where it is special)."""

    def __init__(self, t, q, sp: float, A, B):
        n = len(t)
        self.n, self.ok = n, math.isfinite(sp)
        if not self.ok:
            return
        m = mpmath.mpf
        rd, rv = m(vr.RD), m(vr.RV)
        ph = [m(float(A[k])) + m(float(B[k])) * m(sp) for k in range(n + 1)]
        self.p_half, self.p_full = ph, [(ph[k] + ph[k + 1]) / 2 for k in range(n)]
        self.dphi = [None] * n
        s = m(0)
        for k in range(n - 1, -1, -1):  # bottom level first; dphi is computed once and serves every height
            tk, qk = float(t[k]), float(q[k])
            if not (math.isfinite(tk) and math.isfinite(qk)):
                break
            if k == 0:
                alpha = m(LN2_F64)  # alpha_top = "ifs"
            else:
                lo, hi = ph[k], ph[k + 1]
                if lo == 0 or hi == lo or hi / lo <= 0:
                    break
                alpha = 1 - lo / (hi - lo) * mpmath.log(hi / lo)
            s = s + alpha * (rd * (1 - m(qk)) + rv * m(qk)) * m(tk)
            self.dphi[k] = s

    def count(self, tdphi: float, dphi_numpy) -> int:
        """i = #{k : tdphi > dphi[k]}; numpy's (non-finite) dphi decides at the special levels."""
        return sum(bool(tdphi > (dphi_numpy[k] if d is None else d)) for k, d in enumerate(self.dphi))

    def levels(self, i: int):
        """(a, b) of the count i > 0, as the statement indexes them."""
        n = self.n
        a = n - i - 1
        a = a + n if a < 0 else a  # i == n: numpy's index -1 is the bottom level
        b = 0 if i == n else a + 1
        return a, min(b, n - 1)

    def value(self, tdphi: float, dphi_numpy, special: float):
        """The exact pressure at tdphi = fl64(height * g).  A special dphi enters as numpy's value of it: a NaN gives NaN; an infinite
        dphi[n-1] or dphi[a] makes the interpolation weight 0 (the result is p_half[n] / p_full[b], exact); an infinite dphi[b] gives
        inf / inf.  Where a denominator is zero or the surface pressure is not finite the value is ``special``, numpy's (not finite)."""
        if not self.ok:
            return special
        n, i = self.n, self.count(tdphi, dphi_numpy)
        at = lambda k: float(dphi_numpy[k]) if self.dphi[k] is None else self.dphi[k]  # noqa: E731
        if i == 0:
            d = at(n - 1)
            if isinstance(d, float):
                return math.nan if math.isnan(d) else self.p_half[n]
            if d == 0:
                return special
            return self.p_half[n] + tdphi / d * (self.p_full[n - 1] - self.p_half[n])
        a, b = self.levels(i)
        da, db = at(a), at(b)
        if isinstance(db, float) or (isinstance(da, float) and math.isnan(da)):
            return math.nan if a != b else special
        if isinstance(da, float):
            return self.p_full[b]
        if da == db:
            return special
        return self.p_full[b] + (tdphi - db) / (da - db) * (self.p_full[a] - self.p_full[b])


def tdphi_of(height: float) -> float:
    return float(height) * vr.G


def numpy_dphi(t, q, sp, A, B) -> np.ndarray:
    """The restatement's dphi ``[n_lev, m]`` (float64)."""
    _, _, alpha = vr.pressure_at_model_levels(A, B, sp)
    return vr.relative_geopotential_thickness(alpha, t, q)


def column_exact(heights, t, q, sp, A, B):
    """``(exact, numpy)``: object and float64 arrays ``[len(heights), m]`` of pressure_at_height_levels on the columns of t, q
    ``[n_lev, m]`` and sp ``[m]``."""
    t, q, sp = np.asarray(t), np.asarray(q), np.asarray(sp)
    m = sp.size
    with np.errstate(all="ignore"):
        dphi = numpy_dphi(t, q, sp, A, B)
        want = np.stack([vr.pressure_at_height_levels(h, t, q, sp, A, B) for h in heights])
    exact = np.empty((len(heights), m), dtype=object)
    for c in range(m):
        prof = ColumnProfile(t[:, c], q[:, c], float(sp[c]), A, B)
        for j, h in enumerate(heights):
            x = prof.value(tdphi_of(h), dphi[:, c], float(want[j, c]))
            if isinstance(x, float) and math.isfinite(x):
                raise AssertionError(f"column {c}, height {h}: numpy gives the finite {x} where the exact statement has no value")
            exact[j, c] = x
    return exact, want


def second_walk(dphi: np.ndarray, tdphi: float) -> np.ndarray:
    """Per column of numpy's dphi: 0 < i < n and a = n - 1 - i is not the first level from the bottom that does not count — the
    kernel's `a != a0`, the columns that walk a second time."""
    n = dphi.shape[0]
    counts = tdphi > dphi
    i = counts.sum(axis=0)
    first = n - 1 - np.argmax(~counts[::-1], axis=0)  # (argmax of an all-False column is 0; those columns have i == n)
    return (i > 0) & (i < n) & (n - 1 - i != first)


COLUMN_N_LEV = (1, 2, 3, 60, 137)
# Height classes.  "near ground" is 0, 2 and 10 m — the heights the four filters are used at — and a negative height (i == 0 extended
# below the ground); 100 m is a class of its own: the ill-conditioned alpha of the bottom level enters `below` in proportion to the
# height, and numpy's own error there is ten times that at 10 m, which one class would carry to the heights that matter.
NEAR_GROUND, H100, ALOFT, ABOVE_TOP = "near ground", "100 m", "aloft", "above top"
HEIGHT_CLASSES = (NEAR_GROUND, H100, ALOFT, ABOVE_TOP)
# Case groups: numpy's error on the physical columns and on the bent / special ones (cancellations of a negative layer) differ by
# orders of magnitude, so its worst is pinned — and the kernel's ceiling set — for each
PHYSICAL, ODD = "physical", "bent and special"
CASE_GROUP = {"atmosphere": PHYSICAL, "standard profile": PHYSICAL, "bent": ODD, "specials": ODD}


def _standard_profile(rng, n, m, A, B):
    """A smooth lapse-rate profile in pressure (T = T0 (p / sp)^0.19 down to an isothermal 216.65 K) with 0.2 K of noise; q falls with
    pressure.  dphi is strictly monotone and alpha realistic."""
    sp = rng.uniform(60000.0, 105000.0, m)
    p_full, _, _ = vr.pressure_at_model_levels(A, B, sp)
    t0 = rng.uniform(260.0, 305.0, m)
    t = np.maximum(t0 * (np.maximum(p_full, 1.0) / sp) ** 0.19, 216.65) + rng.normal(0.0, 0.2, (n, m))
    q = np.maximum(rng.uniform(2e-3, 1.8e-2, m) * (p_full / sp) ** 3, 2e-6) * rng.uniform(0.8, 1.2, (n, m))
    return t, q, sp


def _column_heights(n, t, q, sp, A, B):
    """(height, class) pairs: 0, 2, 10, 100 m and one negative height (i == 0, extrapolation below the ground), two interior heights and
    one above the top level, the last three from the median dphi[0] of these columns."""
    with np.errstate(all="ignore"):
        top = float(np.median(numpy_dphi(t, q, sp, A, B)[0])) / vr.G
    return [(0.0, NEAR_GROUND), (2.0, NEAR_GROUND), (10.0, NEAR_GROUND), (100.0, H100), (-2.0, NEAR_GROUND),
            (0.3 * top, ALOFT), (0.7 * top, ALOFT), (1.5 * top + 1000.0, ABOVE_TOP)]


def column_cases(dtype, n_lev: int, seed: int = 0):
    """``(cases, heights)``: {case name: (t[n_lev, m], q[n_lev, m], sp[m])} in ``dtype`` on ``hybrid_column(n_lev)``, and the
    (height, class) pairs every case is evaluated at."""
    rng = np.random.default_rng(1000 * seed + n_lev)
    n = n_lev
    A, B = hybrid_column(n)
    big = n >= 60
    # atmosphere: the ranges of test_height_level_humidity.random_columns, a few dry columns
    m = 160 if big else 256
    t = rng.uniform(200.0, 310.0, (n, m))
    q = 10.0 ** rng.uniform(-6.0, -1.7, (n, m))
    q[:, :7] = 0.0
    atmosphere = (t, q, rng.uniform(50000.0, 106000.0, m))
    standard = _standard_profile(rng, n, 64 if big else 128, A, B)
    heights = _column_heights(n, *standard, A, B)
    # bent: negative temperatures that make dphi non-monotone.  Two thirds of the columns are aimed: a level one to three above the one
    # where dphi first reaches tdphi of a chosen height gets a temperature negative enough to pull dphi under tdphi again, so that
    # level counts, a moves up past it, and the pair (a, a + 1) is no longer the one the first walk kept; the rest carry one to
    # three negative temperatures anywhere (the top included: dphi[0] far below every height).
    m = 96 if big else 128
    bt, bq, bsp = _standard_profile(rng, n, m, A, B)
    with np.errstate(all="ignore"):
        _, _, alpha = vr.pressure_at_model_levels(A, B, bsp)
        term = alpha * (vr.RD * (1.0 - bq) + vr.RV * bq)  # per kelvin
        dphi = numpy_dphi(bt, bq, bsp, A, B)
    aimed = [h for h, _ in heights[1:4]] + [h for h, cls in heights if cls == ALOFT]
    for c in range(m):
        if c % 8 == 7:
            continue  # (a few columns stay straight: the case takes every branch at every n_lev)
        if c % 3 < 2 and n > 1:
            tdphi = tdphi_of(aimed[(c // 3) % len(aimed)])
            below = np.flatnonzero(tdphi > dphi[:, c])
            first = int(below.min()) - 1 if below.size else n - 1  # the first level from the bottom that does not count
            j = max(first - int(rng.integers(1, 4)), 0)
            if j < first or first == 0:
                need = dphi[min(j + 1, n - 1), c] - tdphi  # what the term of level j has to undo
                bt[j, c] = -(max(need, 0.0) / term[j, c]) * rng.uniform(1.2, 3.0) - rng.uniform(1.0, 50.0)
        elif n > 1 or c % 2 == 0:  # (n_lev == 1: every other column, so that both of its branches are taken)
            for j in rng.integers(n, size=int(rng.integers(1, 4))):
                bt[j, c] = -rng.uniform(100.0, 900.0)
    # specials: NaN / +-inf in t or q at the top, the bottom and the middle; NaN, 0, negative and infinite sp; t = 0 at the bottom level
    st, sq, ssp = _standard_profile(rng, n, 24, A, B)
    c = 0
    for arr in (st, sq):
        for level in (0, n - 1, n // 2):
            for v in (np.nan, np.inf, -np.inf):
                if c < 18:
                    arr[level, c] = v
                c += 1
    ssp[18:22] = [np.nan, 0.0, -50000.0, np.inf]
    st[n - 1, 22:24] = 0.0  # dphi[n-1] = 0: 0 / 0 at height 0
    cases = {"atmosphere": atmosphere, "standard profile": standard, "bent": (bt, bq, bsp), "specials": (st, sq, ssp)}
    return _cases(dtype, cases), heights


class ColumnStatement:
    """The column statement on ``column_cases(dtype, n_lev)``: per case the inputs, the exact values and numpy's (float64)
    ``[n_heights, m]``; the errors of a result in ulps of ``dtype`` per case and height."""

    def __init__(self, dtype, n_lev):
        self.dtype, self.n_lev = np.dtype(dtype).type, n_lev
        self.A, self.B = hybrid_column(n_lev)
        self.cases, self.heights = column_cases(dtype, n_lev)
        self.exact, self.numpy_out = {}, {}
        for name, (t, q, sp) in self.cases.items():
            self.exact[name], self.numpy_out[name] = column_exact([h for h, _ in self.heights], t, q, sp, self.A, self.B)
        self._np_err = {}

    def errors(self, case: str, j: int, got: np.ndarray) -> np.ndarray:
        """ulps (of the statement's dtype) of ``got`` from the exact values of height j; the columns may repeat cyclically."""
        x = self.exact[case][j]
        return ulp_errors(got, np.resize(x, np.asarray(got).size), self.dtype)

    def numpy_errors(self, case: str, j: int) -> np.ndarray:
        """numpy's own: the restatement's float64 value, rounded to the statement's dtype."""
        if (case, j) not in self._np_err:
            with np.errstate(all="ignore"):
                self._np_err[case, j] = self.errors(case, j, self.numpy_out[case][j].astype(self.dtype))
        return self._np_err[case, j]

    def numpy_worst(self, cls: str, case: str | None = None, group: str | None = None) -> float:
        """numpy's worst finite error over the heights of a class, on one case, one group of cases, or all."""
        worst = 0.0
        for name in ([case] if case else [c for c in self.cases if group in (None, CASE_GROUP[c])]):
            for j, (_, c) in enumerate(self.heights):
                if c == cls:
                    e = self.numpy_errors(name, j)
                    e = e[np.isfinite(e)]
                    worst = max(worst, float(e.max()) if e.size else 0.0)
        return worst


def column_statement(dtype, n_lev: int) -> ColumnStatement:
    key = ("column", np.dtype(dtype).name, n_lev)
    if key not in _CACHE:
        _CACHE[key] = ColumnStatement(dtype, n_lev)
    return _CACHE[key]
