"""The statement of ``atx_heights_interpolate`` (include/atx_heights.h) restated as a plain loop per (point, variable, target) over numpy
float64 scalars, the same statement in exact arithmetic (mpmath, 240 bits), the comparison the host and the GPU test share, and their
cases.  It shares no code with the package; the columns come from ``geopotential_restatement.make_case``.

For one grid point: sp, zs, the half-level coefficients A[0..H-1], B[0..H-1], the n rows t[0..n-1], q[0..n-1] and x[0..n-1] of each
variable, top first — the LOWEST n model levels: row k is the 0-based level j = first + k, first = H - 1 - n.  A target G is a geopotential
(m^2/s^2) relative to the reference: G = float64(metres) * 9.80665.  Everything in float64, one operation at a time, one rounding to the
stack's type at the end:

    S = 0.0;  z0 = 0.0 ("ground")  or  zs ("sea")
    for k = n - 1 down to 0:          j = first + k
        p_up = A[j] + B[j] * sp       p_dn = A[j + 1] + B[j + 1] * sp
        r = Rd * (1.0 - q[k]) + Rv * q[k]
        j == 0:  alpha = 0.6931471805599453;  no delta
        j  > 0:  delta = log(p_dn / p_up);    alpha = 1.0 - p_up / (p_dn - p_up) * delta
        c[k] = z0 + (S + (alpha * r) * t[k])
        j  > 0:  S = S + (delta * r) * t[k]
    n_below = #{k : c[k] < G}          (the whole column; a NaN c[k] is not below)
    sp != sp or z0 != z0    y = NaN
    n_below == n            "nearest": x[0];  "missing": NaN                                    (above the top full level)
    0 < n_below < n         b = n - n_below, a = b - 1;  w = (c[a] - G) / (c[a] - c[b]);  y = x[a] + w * (x[b] - x[a])
    n_below == 0            c[n - 1] != c[n - 1]: NaN;  G >= z0: x[n - 1]  (the lowest half layer);
                            otherwise "nearest": x[n - 1];  "missing": NaN                      (below the ground)

Errors are measured in ulps (of the case's type) of max(|x[a]|, |x[b]|): y itself can cancel to zero.

``restate(..., defect=)`` plants one of ``DEFECTS`` — a wrong reading of the statement that the comparison must notice.
"""

from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from typing import Optional

import mpmath
import numpy as np

import geopotential_restatement as gr
from hybrid_column_common import assert_same_bits as _assert_same_bits

G = 9.80665
RD, RV, LN2 = gr.RD, gr.RV, gr.LN2
GROUND, SEA = "ground", "sea"
NEAREST, MISSING = "nearest", "missing"
WHOLE, SUBSET = gr.WHOLE, gr.SUBSET
INTERIOR, ABOVE_TOP, LOWEST_HALF_LAYER, BELOW_GROUND, NOT_A_NUMBER = "interior", "above-top", "lowest-half-layer", "below-ground", "nan"
CLASSES = (INTERIOR, ABOVE_TOP, LOWEST_HALF_LAYER, BELOW_GROUND)
DEFECTS = ("count-le", "bottom-first", "weight-flipped", "ground-with-zs", "sea-without-zs", "half-layer-outside", "outside-swapped",
           "targets-in-metres", "first-ignored")
SLACK = 2.0  # ulps the kernel may lose beyond twice numpy's own worst error of the class (levels_restatement.log_budget has the reasoning)
HEIGHTS_M = (-50.0, 2.0, 10.0, 100.0, 200.0, 500.0, 1000.0, 2000.0, 5000.0, 10000.0, 20000.0, 40000.0, 80000.0)
MARGIN = 1e-9  # every exact G is at least this, times |G|, from every exact c[k] of its point: then every correct count is the exact one

# (n_pts, n_lev, kind, n_tgt, n_var, reference): the tile edges (n_pts around 64 and 256), n_var across the variables' buffer, n_tgt > 64
SHAPES = ((0, 3, WHOLE, 13, 1, GROUND), (1, 1, WHOLE, 1, 1, SEA), (63, 2, SUBSET, 13, 3, GROUND), (65, 3, WHOLE, 65, 1, SEA),
          (257, 17, SUBSET, 13, 3, GROUND), (513, 60, WHOLE, 1, 3, SEA), (257, 137, WHOLE, 13, 4, GROUND), (63, 137, SUBSET, 129, 1, SEA))


@dataclass
class HeightsCase:
    name: str
    T: type
    geo: gr.GeoCase               # the N_COLUMNS columns: A, B, sp, t, q (its zs is not read: ``zs`` below is)
    zs: np.ndarray                # [N_COLUMNS] T
    x: np.ndarray                 # [n_pts, n_var, n_lev] T: point p has column p % N_COLUMNS
    heights_m: np.ndarray         # [n_tgt] float64, metres relative to the reference
    reference: str
    geopotentials: Optional[np.ndarray] = None  # [n_tgt] float64: the targets themselves, where they are not float64(h) * g

    @property
    def n_pts(self) -> int:
        return self.x.shape[0]

    @property
    def n_var(self) -> int:
        return self.x.shape[1]

    @property
    def n_lev(self) -> int:
        return self.x.shape[2]

    @property
    def n_tgt(self) -> int:
        return len(self.heights_m)

    @property
    def n_columns(self) -> int:
        return self.geo.n_pts

    @property
    def targets(self) -> np.ndarray:
        """The geopotentials the kernel is handed: float64(h) * g."""
        return self.heights_m.astype(np.float64) * np.float64(G) if self.geopotentials is None else self.geopotentials

    @property
    def kind(self) -> str:
        return self.geo.kind

    def per_point(self, a: np.ndarray) -> np.ndarray:
        """A per-column array repeated cyclically to the case's points."""
        return np.ascontiguousarray(a[np.arange(self.n_pts) % self.n_columns])


# ---- the statement ---------------------------------------------------------------------------------------------------------------
def column(case: HeightsCase, col: int, defect=None) -> tuple[list, np.float64, np.float64]:
    """``(c[0..n-1], z0, sp)`` of column ``col``, numpy float64 scalars."""
    f64 = np.float64
    geo, n = case.geo, case.n_lev
    first = 0 if defect == "first-ignored" else geo.first
    s = f64(geo.sp[col])
    with_zs = defect != "sea-without-zs" if case.reference == SEA else defect == "ground-with-zs"
    z0 = f64(case.zs[col]) if with_zs else f64(0.0)
    c = [None] * n
    S = f64(0.0)
    with np.errstate(all="ignore"):
        for k in range(n - 1, -1, -1):
            j = first + k
            p_up = f64(geo.A[j]) + f64(geo.B[j]) * s
            p_dn = f64(geo.A[j + 1]) + f64(geo.B[j + 1]) * s
            tk, qk = f64(geo.t[col, k]), f64(geo.q[col, k])
            r = f64(RD) * (f64(1.0) - qk) + f64(RV) * qk
            if j == 0:
                alpha, delta = f64(LN2), None
            else:
                delta = np.log(p_dn / p_up)
                alpha = f64(1.0) - p_up / (p_dn - p_up) * delta
            c[k] = z0 + (S + (alpha * r) * tk)
            if delta is not None:
                S = S + (delta * r) * tk
    return c, z0, s


def bracket(c: list, z0, s, target, outside, defect=None):
    """``(kind, a, b, w)`` of one (column, target): kind is one of CLASSES or NOT_A_NUMBER; a is None where the result is NaN, a == b a copy."""
    n = len(c)
    target = np.float64(target)
    if defect == "outside-swapped":
        outside = MISSING if outside == NEAREST else NEAREST
    if s != s or z0 != z0:
        return NOT_A_NUMBER, None, None, None
    n_below = 0
    for ck in c:
        if (ck <= target) if defect == "count-le" else (ck < target):
            n_below += 1
    if n_below == n:
        return (ABOVE_TOP, 0, 0, None) if outside == NEAREST else (ABOVE_TOP, None, None, None)
    if n_below > 0:
        b = n - n_below
        a = b - 1
        with np.errstate(all="ignore"):
            w = (target - c[b]) / (c[a] - c[b]) if defect == "weight-flipped" else (c[a] - target) / (c[a] - c[b])
        return INTERIOR, a, b, w
    if c[n - 1] != c[n - 1]:
        return NOT_A_NUMBER, None, None, None
    if target >= z0 and defect != "half-layer-outside":
        return LOWEST_HALF_LAYER, n - 1, n - 1, None
    return (BELOW_GROUND, n - 1, n - 1, None) if outside == NEAREST else (BELOW_GROUND, None, None, None)


def element(x_column, a, b, w) -> np.float64:
    """y of one (point, variable, target) before the rounding to the stack's type: ``x_column`` is the variable's n rows."""
    if a is None:
        return np.float64(np.nan)
    if a == b:
        return np.float64(x_column[a])
    xa, xb = np.float64(x_column[a]), np.float64(x_column[b])
    with np.errstate(all="ignore"):
        return xa + w * (xb - xa)


def brackets(case: HeightsCase, outside=NEAREST, defect=None) -> list:
    """``[column][target]`` of ``bracket`` results: a point's bracket is its column's."""
    targets = case.heights_m.astype(np.float64) if defect == "targets-in-metres" else case.targets
    out = []
    for col in range(min(case.n_columns, case.n_pts)):
        c, z0, s = column(case, col, defect)
        out.append([bracket(c, z0, s, target, outside, defect) for target in targets])
    return out


def restate(case: HeightsCase, outside=NEAREST, defect=None, rounded=True) -> np.ndarray:
    """``[n_pts, n_var, n_tgt]`` in the case's type (``rounded=False``: the float64 values before the store)."""
    out = np.empty((case.n_pts, case.n_var, case.n_tgt), dtype=np.float64)
    found = brackets(case, outside, defect)
    for p in range(case.n_pts):
        for v in range(case.n_var):
            x_column = case.x[p, v, ::-1] if defect == "bottom-first" else case.x[p, v]
            for i in range(case.n_tgt):
                _, a, b, w = found[p % case.n_columns][i]
                out[p, v, i] = element(x_column, a, b, w)
    if not rounded:
        return out
    with np.errstate(all="ignore"):
        return out.astype(case.T)


def classes(case: HeightsCase, outside=NEAREST) -> np.ndarray:
    """``[columns, n_tgt]`` of class names."""
    return np.array([[entry[0] for entry in row] for row in brackets(case, outside)], dtype=object).reshape(-1, case.n_tgt)


# ---- the same statement, exact -----------------------------------------------------------------------------------------------------
def ulp_of(r, T) -> mpmath.mpf:
    """One ulp of the magnitude ``r`` in the type T (normal range: the cases here stay inside it)."""
    precision = 24 if np.dtype(T) == np.float32 else 53
    return mpmath.ldexp(1, mpmath.frexp(r)[1] - precision)


def exact_column(case: HeightsCase, col: int):
    """``(c[0..n-1], z0)`` of the column with mpmath, None where the statement's value is not a finite number; ``None`` for a column
    whose sp or z0 is not a number."""
    mp = mpmath.mpf
    geo, n = case.geo, case.n_lev
    s = float(geo.sp[col])
    z0 = float(case.zs[col]) if case.reference == SEA else 0.0
    if s != s or z0 != z0:
        return None
    c = [None] * n
    if not (math.isfinite(s) and math.isfinite(z0)):
        return c, mp(0)
    s, z0 = mp(s), mp(z0)
    rd, rv, ln2 = mp(RD), mp(RV), mpmath.log(2)
    S = mp(0)
    for k in range(n - 1, -1, -1):
        j = geo.first + k
        tk, qk = float(geo.t[col, k]), float(geo.q[col, k])
        if not (math.isfinite(tk) and math.isfinite(qk)):
            break  # this level and every level above it
        p_up, p_dn = mp(float(geo.A[j])) + mp(float(geo.B[j])) * s, mp(float(geo.A[j + 1])) + mp(float(geo.B[j + 1])) * s
        r = rd * (1 - mp(qk)) + rv * mp(qk)
        if j == 0:
            alpha, delta = ln2, mp(0)
        else:
            if not (p_up > 0 and p_dn > p_up):
                break
            delta = mpmath.log(p_dn / p_up)
            alpha = 1 - p_up / (p_dn - p_up) * delta
        c[k] = z0 + (S + alpha * r * mp(tk))
        S = S + delta * r * mp(tk)
    return c, z0


def exact_brackets(case: HeightsCase, with_margins: bool = False) -> list:
    """``[column][target]``: ``(a, b, w)`` of the exact interior brackets — exact c, exact count, exact weight — None elsewhere; and
    beside it, ``with_margins``, the smallest |G - c[k]| / |G| over the column's levels (None for a column without numbers)."""
    import bisect

    mp = mpmath.mpf
    out = []
    with mpmath.workprec(240):
        for col in range(min(case.n_columns, case.n_pts)):
            found = exact_column(case, col)
            numbers = sorted(ck for ck in found[0] if ck is not None) if found is not None else []
            row = []
            for h in case.targets:
                if found is None:
                    row.append((None, None))
                    continue
                c, _ = found
                target = mp(float(h))  # the float64 the kernel is handed, exactly
                margin = None
                if with_margins and target != 0 and numbers:
                    margin = min(abs(target - ck) / abs(target) for ck in numbers)
                n, n_below = len(c), bisect.bisect_left(numbers, target)  # #{k : c[k] < G} over the levels that are numbers
                if 0 < n_below < n and c[n - n_below - 1] is not None and c[n - n_below] is not None:
                    b = n - n_below
                    a = b - 1
                    row.append(((a, b, (c[a] - target) / (c[a] - c[b])), margin))
                else:
                    row.append((None, margin))
            out.append(row)
    return out


def exact(case: HeightsCase) -> tuple[np.ndarray, np.ndarray]:
    """``(value, unit)``, both ``[n_pts, n_var, n_tgt]`` object arrays, for the INTERIOR elements with a finite bracket (None elsewhere):
    the statement evaluated with mpmath from the same inputs, and one ulp of max(|x[a]|, |x[b]|) in the case's type."""
    mp = mpmath.mpf
    value = np.full((case.n_pts, case.n_var, case.n_tgt), None, dtype=object)
    unit = np.full((case.n_pts, case.n_var, case.n_tgt), None, dtype=object)
    found = exact_bracket_reference(case)
    with mpmath.workprec(240):
        for p in range(case.n_pts):
            for i in range(case.n_tgt):
                interior = found[p % case.n_columns][i][0]
                if interior is None:
                    continue
                a, b, w = interior
                for v in range(case.n_var):
                    xa, xb = float(case.x[p, v, a]), float(case.x[p, v, b])
                    if not (math.isfinite(xa) and math.isfinite(xb)) or max(abs(xa), abs(xb)) == 0.0:
                        continue
                    value[p, v, i] = mp(xa) + w * (mp(xb) - mp(xa))
                    unit[p, v, i] = ulp_of(max(abs(xa), abs(xb)), case.T)
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


def margins(case: HeightsCase) -> tuple[float, int]:
    """``(the smallest |G - c[k]| / |G| of the case, exact; the (column, target) pairs whose numpy bracket is not the exact one)``."""
    found, numpy_found = exact_brackets(case, with_margins=True), brackets(case)
    smallest, disagreements = math.inf, 0
    for col, row in enumerate(found):
        for i, (interior, margin) in enumerate(row):
            if margin is not None:
                smallest = min(smallest, float(margin))
            kind, a, b, w = numpy_found[col][i]
            numpy_interior = kind == INTERIOR and bool(np.isfinite(w))  # (a bracket that holds a NaN level has no exact value)
            if (interior is not None) != numpy_interior or (interior is not None and (a, b) != interior[:2]):
                disagreements += 1
    return smallest, disagreements


def numpy_worst(case: HeightsCase) -> float:
    """numpy's float64 arithmetic (the restatement before its rounding) against exact, in FLOAT64 ulps of max(|x[a]|, |x[b]|), whatever
    the case's type."""
    value, unit = exact_reference(case)
    scale = 2.0**-29 if case.T is np.float32 else 1.0
    e = errors(reference(case, NEAREST, rounded=False), value, unit, scale)
    return float(np.nanmax(e)) if (~np.isnan(e)).any() else 0.0


# ---- the comparison of the GPU test (plain functions: the host test drives them with planted defects) -------------------------------
assert_same_bits = functools.partial(_assert_same_bits, axes="(point, variable, target)")


def bound(case: HeightsCase, numpy_pinned: float) -> float:
    """The rule of ``levels_restatement.log_budget`` with numpy's PINNED worst error of the class, in ulps of max(|x[a]|, |x[b]|) of the
    case's type.  float64: twice numpy's worst plus SLACK — kernel and numpy evaluate the same statements in the same order with IEEE
    operations, the one primitive that differs is the logarithm (the library's is budgeted at 1 ulp, glibc's is at about half that), so
    the kernel may carry up to twice numpy's share.  float32: the float64 arithmetic under that bound (one float64 ulp is 2^-29 float32
    ulps) and one rounding at the store, 0.5 ulp of y, which is at most 0.5 ulp of max(|x[a]|, |x[b]|) wherever w is inside [0, 1] — in
    every column whose c never increases towards the ground."""
    ceiling = 2.0 * numpy_pinned + SLACK
    return 0.5 + ceiling * 2.0**-29 if case.T is np.float32 else ceiling


def check(compute, cases, pinned, report=None, accuracy=True) -> None:
    """``compute(case, outside)`` -> ``[n_pts, n_var, n_tgt]`` of the case's type, under both policies: NaN and infinities exactly where
    the restatement has them; what the statement copies (outside, the lowest half layer) bit for bit; under "nearest" every finite
    interior value within ``bound`` of the exact statement, and under "missing" the bits of "nearest" there.  ``pinned``: numpy's worst
    per (n_lev, kind, reference), or a function of the case that gives it.  ``accuracy=False`` leaves the bound out (a float32 case whose
    columns are not monotone: the rule's precondition does not hold)."""
    for case in cases:
        value, unit = exact_reference(case)
        interior = np.vectorize(lambda v: v is not None, otypes=[bool])(value)
        results = {}
        for outside in (NEAREST, MISSING):
            want = reference(case, outside)
            got = results[outside] = compute(case, outside)
            what = f"{case.name} {outside}"
            assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape)
            assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN positions differ at (point, variable, target) {np.argwhere(np.isnan(got) != np.isnan(want))[:5].tolist()}"
            inf = np.isinf(want)
            assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]), f"{what}: infinities differ"
            copied = ~interior & ~np.isnan(want)
            assert_same_bits(np.where(copied, got, 0).astype(got.dtype), np.where(copied, want, 0).astype(got.dtype), what + " (copies)")
        if case.n_pts == 0:
            continue
        near, miss = results[NEAREST], results[MISSING]
        assert_same_bits(np.where(interior, miss, 0).astype(miss.dtype), np.where(interior, near, 0).astype(near.dtype), f"{case.name}: interior, missing against nearest")
        if not accuracy:
            continue
        e = errors(near, value, unit)
        worst_numpy = pinned(case) if callable(pinned) else pinned[(case.n_lev, case.kind, case.reference)]
        limit = bound(case, worst_numpy)
        worst = float(np.nanmax(e)) if (~np.isnan(e)).any() else 0.0
        if report is not None:
            report[case.name] = dict(kernel=worst, numpy_float64=numpy_worst(case), bound=limit)
        assert worst <= limit, (f"{case.name}: {worst:.4f} ulps of max(|x[a]|, |x[b]|) from exact > {limit:.6g} at (point, variable, target) "
                                f"{np.argwhere(e > limit)[:5].tolist()}")


# references are computed once per case and shared; nothing changes them
_REFERENCES: dict = {}


def reference(case: HeightsCase, outside=NEAREST, rounded=True) -> np.ndarray:
    key = (case.name, outside, rounded)
    if key not in _REFERENCES:
        _REFERENCES[key] = restate(case, outside, rounded=rounded)
        _REFERENCES[key].setflags(write=False)
    return _REFERENCES[key]


def exact_bracket_reference(case: HeightsCase):
    key = (case.name, "exact-brackets")
    if key not in _REFERENCES:
        _REFERENCES[key] = exact_brackets(case)
    return _REFERENCES[key]


def exact_reference(case: HeightsCase):
    key = (case.name, "exact")
    if key not in _REFERENCES:
        _REFERENCES[key] = exact(case)
    return _REFERENCES[key]


# ---- cases -----------------------------------------------------------------------------------------------------------------------
def heights_of(n_tgt: int, rng) -> np.ndarray:
    """The heights of a case, metres: HEIGHTS_M for 13 targets, 100 m alone, and for more the thirteen, random ones between 1 m and
    60 km behind them and a duplicate of the fourth at the end — in no order."""
    if n_tgt == 1:
        return np.array([100.0])
    if n_tgt <= len(HEIGHTS_M):
        return np.array(HEIGHTS_M[:n_tgt])
    extra = np.exp(rng.uniform(np.log(1.0), np.log(60000.0), n_tgt - len(HEIGHTS_M) - 1))
    return np.array(list(HEIGHTS_M) + [float(v) for v in extra] + [HEIGHTS_M[3]])


@functools.lru_cache(maxsize=None)
def make_case(T, n_pts: int, n_lev: int, kind: str, n_tgt: int, n_var: int, reference: str, specials: bool = True) -> HeightsCase:
    """The columns of ``gr.make_case`` (with zs), repeated cyclically to ``n_pts`` points; x random around 250 with, where the case has
    the points for it, one NaN mid-column (point 9), -inf at the bottom (point 10) and +inf at the top (point 11); ``specials``: those of
    the columns (NaN and inf in t and q, a NaN sp) and a NaN zs (column 8), which only the sea reference reads.  Above the sea the heights
    are those above the ground plus the case's median zs / g."""
    geo = gr.make_case(T, n_lev, kind, True, specials)
    rng = np.random.default_rng([20261021, n_pts, n_lev, kind == SUBSET, n_tgt, n_var, reference == SEA, np.dtype(T).itemsize])
    x = (250.0 + 30.0 * rng.standard_normal((n_pts, n_var, n_lev))).astype(T)
    if n_pts > 11:
        x[9, 0, n_lev // 2] = np.nan
        x[10, n_var - 1, n_lev - 1] = -np.inf
        x[11, 0, 0] = np.inf
    zs = geo.zs.copy()
    if specials:
        zs[8] = np.nan
    heights = heights_of(n_tgt, rng)
    if reference == SEA:
        heights = heights + float(np.nanmedian(zs.astype(np.float64)) / G)
    name = f"{kind}-{n_pts}x{n_var}x{n_lev}-to-{n_tgt}-{reference}-{np.dtype(T).name}" + ("" if specials else "-finite")
    return HeightsCase(name, T, geo, zs, x, heights, reference)


def shape_cases(T) -> list:
    return [make_case(T, *shape) for shape in SHAPES]


def on_level_case(T=np.float64) -> HeightsCase:
    """A case for the host test alone: targets that ARE numpy's c[k] of a column — its top, its bottom and a level in between — where
    the count's `<` against `<=` decides.  (A kernel's c may differ from numpy's in its last bits: no GPU test takes this case.)"""
    base = make_case(T, 48, 17, WHOLE, 13, 2, GROUND, False)
    chosen = [column(base, col)[0][k] for col, k in ((0, 0), (0, 16), (12, 8), (20, 0), (20, 16), (33, 5))]
    targets = np.array([float(ck) for ck in chosen] + [150.0 * G])
    return HeightsCase("on-level-" + np.dtype(T).name, T, base.geo, base.zs, base.x, targets / G, GROUND, targets)


def bent_case(T, n_pts: int = 65, reference: str = SEA) -> HeightsCase:
    """Columns whose c is NOT monotone: a few negative t (columns 9 .. 20, two levels each) — the whole-column count runs there."""
    base = make_case(T, n_pts, 17, WHOLE, 13, 2, reference)
    t = base.geo.t.copy()
    for col in range(9, 21):
        t[col, 5], t[col, 11] = -t[col, 5], -3.0 * t[col, 11]
    geo = gr.GeoCase(base.geo.name + "-bent", T, base.geo.A, base.geo.B, base.geo.sp, base.geo.zs, t, base.geo.q)
    return HeightsCase("bent-" + base.name, T, geo, base.zs, base.x, base.heights_m, reference)
