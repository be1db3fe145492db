"""The statement of ``atx_geopotential_on_model_levels`` (include/atx_geopotential.h) restated as a plain loop per point over numpy float64 scalars, the
same statement in exact arithmetic (mpmath) from the same inputs, the comparisons the GPU test uses, and the cases the host and GPU tests
share.  It shares no code with the package.

For one grid point: surface pressure sp, surface geopotential zs (None: 0.0), half-level coefficients A[0..H-1], B[0..H-1], the n rows
t[0..n-1], q[0..n-1], top first — the LOWEST n model levels: row k is the 0-based level j = first + k, first = H - 1 - n.  Everything in
float64, one operation at a time, one rounding to the stack's type at the end:

    S = 0.0
    for k = n - 1 down to 0:          j = first + k
        p_up = A[j] + B[j] * sp       p_dn = A[j + 1] + B[j + 1] * sp
        r = Rd * (1.0 - q[k]) + Rv * q[k]
        j == 0:  alpha = 0.6931471805599453;  no delta
        j  > 0:  delta = log(p_dn / p_up);    alpha = 1.0 - p_up / (p_dn - p_up) * delta
        z[k] = zs + (S + (alpha * r) * t[k])
        j  > 0:  S = S + (delta * r) * t[k]

Errors are measured in ulps (of the case's type) of U[k] = |zs| + sum over the levels below of |delta r t| + |alpha r t|: the magnitude
the sum passes through — z itself can cancel against a negative zs.

``restate(..., defect=)`` plants one of ``DEFECTS`` — a wrong reading of the statement that the comparisons must notice.
"""

from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from typing import Optional

import mpmath
import numpy as np

from hybrid_column_common import assert_same_bits as _assert_same_bits, bits_type, eta_table  # noqa: F401 - the tests reach them here

RD, RV = 287.0597, 461.5250
LN2 = 0.6931471805599453
DEFECTS = ("alpha-only", "own-delta", "top-first", "dry", "zs-dropped", "first-ignored", "top-general")
SLACK = 2.0  # ulps the kernel may lose beyond twice numpy's own worst error of the class (tests/test_gpu_column_ulps.py has the reasoning)
WHOLE, SUBSET = "whole", "subset"
N_COLUMNS = 48  # the columns of a case; a test that wants more points repeats them cyclically (``expand``)
SUBSET_ABOVE = 8  # a subset case leaves out this many levels at the top of its table
N_LEVS = (1, 2, 3, 60, 137)
# (n_lev, kind, n_pts, zs): every n_lev whole and subset, every n_pts of {1, 63, 65, 257, 513} twice, zs NULL four times
SHAPES = ((1, WHOLE, 1, True), (1, SUBSET, 63, True), (2, WHOLE, 65, False), (2, SUBSET, 257, True), (3, WHOLE, 513, True),
          (3, SUBSET, 1, False), (60, WHOLE, 257, True), (60, SUBSET, 65, False), (137, WHOLE, 513, True), (137, SUBSET, 63, False))


@dataclass
class GeoCase:
    name: str
    T: type
    A: np.ndarray                 # [H] float64
    B: np.ndarray                 # [H] float64
    sp: np.ndarray                # [n_pts] T
    zs: Optional[np.ndarray]      # [n_pts] T, or None: 0.0 everywhere
    t: np.ndarray                 # [n_pts, n_lev] T
    q: np.ndarray                 # [n_pts, n_lev] T

    @property
    def n_pts(self) -> int:
        return self.t.shape[0]

    @property
    def n_lev(self) -> int:
        return self.t.shape[1]

    @property
    def n_half(self) -> int:
        return len(self.A)

    @property
    def first(self) -> int:
        return self.n_half - 1 - self.n_lev

    @property
    def kind(self) -> str:
        return WHOLE if self.first == 0 else SUBSET


# ---- the statement ---------------------------------------------------------------------------------------------------------------
def column(case: GeoCase, p: int, defect=None) -> list:
    """z[0..n-1] of point p, numpy float64 scalars (before the rounding to the case's type)."""
    f64 = np.float64
    n = case.n_lev
    first = 0 if defect == "first-ignored" else case.first
    s = f64(case.sp[p])
    zs = f64(0.0) if case.zs is None or defect == "zs-dropped" else f64(case.zs[p])
    t, q = case.t[p], case.q[p]
    if defect == "top-first":
        t, q = t[::-1], q[::-1]
    z = [None] * n
    S = f64(0.0)
    with np.errstate(all="ignore"):
        for k in range(n - 1, -1, -1):
            j = first + k
            p_up = f64(case.A[j]) + f64(case.B[j]) * s
            p_dn = f64(case.A[j + 1]) + f64(case.B[j + 1]) * s
            tk, qk = f64(t[k]), f64(q[k])
            r = f64(RD) if defect == "dry" else f64(RD) * (f64(1.0) - qk) + f64(RV) * qk
            if j == 0 and defect != "top-general":
                alpha, delta = f64(LN2), None
            else:
                delta = np.log(p_dn / p_up)
                alpha = f64(1.0) - p_up / (p_dn - p_up) * delta
            own = (delta if defect == "own-delta" and delta is not None else alpha) * r * tk
            z[k] = zs + (S + own)
            if delta is not None:
                S = S + ((alpha if defect == "alpha-only" else delta) * r) * tk
    return z


def restate(case: GeoCase, defect=None, rounded=True) -> np.ndarray:
    """``[n_pts, n_lev]`` in the case's type (``rounded=False``: the float64 values before the store)."""
    out = np.array([column(case, p, defect) for p in range(case.n_pts)], dtype=np.float64).reshape(case.n_pts, case.n_lev)
    if not rounded:
        return out
    with np.errstate(all="ignore"):
        return out.astype(case.T)


# ---- the same statement, exact -----------------------------------------------------------------------------------------------------
def ulp_of(r, T) -> mpmath.mpf:
    """One ulp of the magnitude ``r`` in the type T (normal range: the cases here stay inside it)."""
    precision = 24 if np.dtype(T) == np.float32 else 53
    return mpmath.ldexp(1, mpmath.frexp(r)[1] - precision)


def exact(case: GeoCase) -> tuple[np.ndarray, np.ndarray]:
    """``(value, unit)``, both ``[n_pts, n_lev]`` object arrays: the statement evaluated with mpmath from the same inputs and one ulp of
    U[k] in the case's type — None where the statement's value is not a finite number (a NaN or an infinity among what feeds it)."""
    mp = mpmath.mpf
    value = np.full((case.n_pts, case.n_lev), None, dtype=object)
    unit = np.full((case.n_pts, case.n_lev), None, dtype=object)
    with mpmath.workprec(240):
        rd, rv, ln2 = mp(RD), mp(RV), mpmath.log(2)
        for p in range(case.n_pts):
            s, zs = float(case.sp[p]), 0.0 if case.zs is None else float(case.zs[p])
            if not math.isfinite(zs):
                continue
            sp_is_a_number = math.isfinite(s)
            s, zs = mp(s if sp_is_a_number else 0.0), mp(zs)
            S, U = mp(0), abs(zs)
            for k in range(case.n_lev - 1, -1, -1):
                j = case.first + k
                tk, qk = float(case.t[p, k]), float(case.q[p, k])
                if not (math.isfinite(tk) and math.isfinite(qk)) or not (sp_is_a_number or j == 0):
                    break  # this level and every level above it (model level 0 alone reads no pressure)
                p_up, p_dn = mp(float(case.A[j])) + mp(float(case.B[j])) * s, mp(float(case.A[j + 1])) + mp(float(case.B[j + 1])) * s
                r = rd * (1 - mp(qk)) + rv * mp(qk)
                if j == 0:
                    alpha, delta = ln2, mp(0)
                else:
                    if not (p_up > 0 and p_dn > p_up):
                        break
                    delta = mpmath.log(p_dn / p_up)
                    alpha = 1 - p_up / (p_dn - p_up) * delta
                own = alpha * r * mp(tk)
                value[p, k] = zs + S + own
                magnitude = U + abs(own)
                if magnitude > 0:
                    unit[p, k] = ulp_of(magnitude, case.T)
                else:
                    value[p, k] = None
                S, U = S + delta * r * mp(tk), U + abs(delta * r * mp(tk))
    return value, unit


def errors(got: np.ndarray, value: np.ndarray, unit: np.ndarray, unit_scale: float = 1.0) -> np.ndarray:
    """|got - exact| in the units of ``exact`` times ``unit_scale`` (NaN where there is no exact value; inf where ``got`` is not finite
    there)."""
    out = np.full(got.shape, np.nan)
    with mpmath.workprec(240):
        for idx in np.ndindex(got.shape):
            if value[idx] is None:
                continue
            g = float(got[idx])
            out[idx] = float(abs(mpmath.mpf(g) - value[idx]) / (unit[idx] * unit_scale)) if math.isfinite(g) else math.inf
    return out


def numpy_worst(case: GeoCase) -> float:
    """numpy's float64 arithmetic (the restatement before its rounding) against exact, in FLOAT64 ulps of U, whatever the case's type."""
    value, unit = exact_reference(case)
    scale = 2.0**-29 if case.T is np.float32 else 1.0
    e = errors(reference(case, rounded=False), value, unit, scale)
    return float(np.nanmax(e)) if (~np.isnan(e)).any() else 0.0


# ---- the comparisons of the GPU test (plain functions: the host test drives them with planted defects) ------------------------------
assert_same_bits = functools.partial(_assert_same_bits, axes="(point, level)")


def has_logarithm(case: GeoCase) -> bool:
    return not (case.n_lev == 1 and case.first == 0)


def ceiling64(numpy_pinned: float) -> float:
    """The float64 bound of a class from numpy's PINNED worst error of it: kernel and numpy evaluate the same statements in the same
    order with IEEE operations; the one primitive that differs is the logarithm (the library's is budgeted at 1 ulp, glibc's is at about
    half that), so the kernel may carry up to twice numpy's share, and SLACK."""
    return 2.0 * numpy_pinned + SLACK


def bound(case: GeoCase, numpy_pinned: float) -> float:
    """In ulps of U of the case's type.  float32: the float64 arithmetic under the float64 ceiling (one float64 ulp is 2^-29 float32
    ulps) and one rounding at the store: 0.5 ulp of z, and |z| <= U."""
    c = ceiling64(numpy_pinned)
    return 0.5 + c * 2.0**-29 if case.T is np.float32 else c


def check(compute, cases, pinned: dict, report=None) -> None:
    """``compute(case)`` -> ``[n_pts, n_lev]`` of the case's type: NaN and infinities exactly where the restatement has them; a case
    without a logarithm (model level 0 alone) bit for bit; in every other case each finite value within ``bound`` of the exact statement.
    ``pinned``: numpy's worst per (n_lev, kind)."""
    for case in cases:
        want = reference(case)
        got = compute(case)
        what = case.name
        assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape)
        assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN positions differ at (point, level) {np.argwhere(np.isnan(got) != np.isnan(want))[:5].tolist()}"
        inf = np.isinf(want)
        assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]), f"{what}: infinities differ"
        if not has_logarithm(case):
            assert_same_bits(got, want, what + " (no logarithm)")
            continue
        value, unit = exact_reference(case)
        e = errors(got, value, unit)
        limit = bound(case, pinned[(case.n_lev, case.kind)])
        worst = float(np.nanmax(e)) if (~np.isnan(e)).any() else 0.0
        if report is not None:
            report[case.name] = dict(kernel=worst, numpy_float64=numpy_worst(case), bound=limit)
        assert worst <= limit, f"{what}: {worst:.4f} ulps of U from exact > {limit:.6g} at (point, level) {np.argwhere(e > limit)[:5].tolist()}"


# references are computed once per case and shared; nothing changes them
_REFERENCES: dict = {}


def reference(case: GeoCase, rounded=True) -> np.ndarray:
    key = (case.name, rounded)
    if key not in _REFERENCES:
        _REFERENCES[key] = restate(case, rounded=rounded)
        _REFERENCES[key].setflags(write=False)
    return _REFERENCES[key]


def exact_reference(case: GeoCase):
    key = (case.name, "exact")
    if key not in _REFERENCES:
        _REFERENCES[key] = exact(case)
    return _REFERENCES[key]


def expand(a: Optional[np.ndarray], n_pts: int) -> Optional[np.ndarray]:
    """The first axis repeated cyclically to ``n_pts`` entries."""
    return None if a is None else np.ascontiguousarray(a[np.arange(n_pts) % a.shape[0]])


# ---- cases -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def make_case(T, n_lev: int, kind: str = WHOLE, with_zs: bool = True, specials: bool = True) -> GeoCase:
    """N_COLUMNS random columns: t around 250 K, q in [0, 0.02], sp in [50 000, 105 000] Pa, zs in [-500, 30 000] with one strongly
    negative and one large value.  ``specials``: a NaN planted mid-column in t (column 1) and in q (column 5), +inf at the top of t
    (column 2), -inf at the bottom of q (column 3) and a NaN sp (column 4)."""
    rng = np.random.default_rng([20261021, n_lev, kind == SUBSET, with_zs, np.dtype(T).itemsize])
    A, B = eta_table(n_lev + 1 + (SUBSET_ABOVE if kind == SUBSET else 0))
    n = N_COLUMNS
    sp = rng.uniform(50000.0, 105000.0, n).astype(T)
    t = (250.0 + 30.0 * rng.standard_normal((n, n_lev))).astype(T)
    q = rng.uniform(0.0, 0.02, (n, n_lev)).astype(T)
    zs = rng.uniform(-500.0, 30000.0, n).astype(T) if with_zs else None
    if with_zs:
        zs[6], zs[7] = -4.0e4, 3.0e6  # z cancels against the first; the second swamps the sum
    if specials:
        mid = n_lev // 2
        t[1, mid] = np.nan
        t[2, 0] = np.inf
        q[3, n_lev - 1] = -np.inf
        sp[4] = np.nan
        q[5, mid] = np.nan
    name = f"{kind}-{n_lev}-{'zs' if with_zs else 'nozs'}-{np.dtype(T).name}" + ("" if specials else "-finite")
    return GeoCase(name, T, A, B, sp, zs, t, q)


def shape_cases(T) -> list:
    """The case of every entry of SHAPES (its n_pts is the GPU test's business: ``expand``)."""
    return [make_case(T, n_lev, kind, with_zs) for n_lev, kind, _, with_zs in SHAPES]
