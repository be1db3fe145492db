"""The statement of ``atx_levels_interpolate`` (include/atx_levels.h) restated as a plain loop per (point, variable, target) over numpy
float64 scalars, the same statement in exact arithmetic (mpmath), the comparisons the GPU test uses, and the cases the host and GPU tests
share.  It shares no code with the package.

For one grid point: surface pressure sp, half-level coefficients A[0..H-1], B[0..H-1], the n rows x[0..n-1] of a variable, top first, each
row's 0-based model level m[k] (strictly increasing; k itself without a level index).  Everything in float64, one operation at a time, one
rounding to the stack's type at the end:

    p_half(j) = A[j] + B[j] * sp
    p_full[k] = (p_half(m[k]) + p_half(m[k] + 1)) / 2
    p_ground  = p_half(H - 1)
    c(p)      = p ("linear")  or  log(p) ("log")
    i = #{k : p_full[k] <= P}          (the whole column; a NaN sp gives 0, and the result is NaN under every policy)
    0 < i < n               a = i - 1, b = i;  w = (c(P) - c(p_full[a])) / (c(p_full[b]) - c(p_full[a]));  y = x[a] + w * (x[b] - x[a])
    i == n, P <= p_ground   y = x[n - 1]                    (the half layer above the ground)
    i == n otherwise        "nearest": x[n - 1];  "missing": NaN      (below the ground)
    i == 0                  "nearest": x[0];      "missing": NaN      (above the top full level)

``restate(..., defect=)`` plants one of ``DEFECTS`` — a wrong reading of the statement that the comparisons must notice.
"""

from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from typing import Optional

import mpmath
import numpy as np

import exact_statements as X
from hybrid_column_common import assert_same_bits as _assert_same_bits, bits_type, eta_table  # noqa: F401 - the tests reach them here

LINEAR, LOG = "linear", "log"
NEAREST, MISSING = "nearest", "missing"
INTERIOR, ABOVE_TOP, LOWEST_HALF_LAYER, BELOW_GROUND, NAN_SP = "interior", "above-top", "lowest-half-layer", "below-ground", "nan-sp"
CLASSES = (INTERIOR, ABOVE_TOP, LOWEST_HALF_LAYER, BELOW_GROUND)
DEFECTS = ("half-levels", "count-lt", "bottom-first", "outside-swapped", "weight-in-p", "ground-is-sp", "level-index-ignored")
SLACK = 2.0  # ulps the kernel may lose beyond twice numpy's own worst error on the same case (tests/test_gpu_ulp_budgets.py)

BASE_SEED = 20261021
BASE_TARGETS = (100.0, 1000.0, 5000.0, 20000.0, 50000.0, 70000.0, 85000.0, 92500.0, 100000.0, 110000.0)


@dataclass
class LevelsCase:
    name: str
    T: type
    A: np.ndarray                 # [H] float64
    B: np.ndarray                 # [H] float64
    m: Optional[np.ndarray]       # [n_lev] the rows' model levels, or None: 0 .. n_lev - 1
    sp: np.ndarray                # [n_pts] T
    x: np.ndarray                 # [n_pts, n_var, n_lev] T
    targets: np.ndarray           # [n_tgt] float64, Pa

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
        return len(self.targets)

    def levels(self) -> list[int]:
        return list(range(self.n_lev)) if self.m is None else [int(v) for v in self.m]


# ---- the statement ---------------------------------------------------------------------------------------------------------------
def full_levels(case: LevelsCase, p: int, defect=None) -> tuple[list, np.float64, np.float64]:
    """(p_full[0..n-1], p_ground, sp) of point p, numpy float64 scalars."""
    A, B = case.A, case.B
    s = np.float64(case.sp[p])
    levels = list(range(case.n_lev)) if defect == "level-index-ignored" else case.levels()
    with np.errstate(all="ignore"):
        def half(j):
            return np.float64(A[j]) + np.float64(B[j]) * s

        if defect == "half-levels":
            pf = [half(j + 1) for j in levels]
        else:
            pf = [(half(j) + half(j + 1)) / np.float64(2.0) for j in levels]
        ground = s if defect == "ground-is-sp" else half(len(A) - 1)
    return pf, ground, s


def bracket(pf: list, ground, s, P, coordinate, outside, defect=None):
    """``(kind, a, b, w)`` of one (point, target): kind is one of CLASSES or NAN_SP; a is None where the result is NaN, a == b a copy."""
    n = len(pf)
    P = np.float64(P)
    if defect == "outside-swapped":
        outside = MISSING if outside == NEAREST else NEAREST
    if s != s:
        return NAN_SP, None, None, None
    i = 0
    for pk in pf:
        if (pk < P) if defect == "count-lt" else (pk <= P):
            i += 1
    if 0 < i < n:
        a, b = i - 1, i
        with np.errstate(all="ignore"):
            if coordinate == LOG and defect != "weight-in-p":
                ca, cb, cp = np.log(pf[a]), np.log(pf[b]), np.log(P)
            else:
                ca, cb, cp = pf[a], pf[b], P
            w = (cp - ca) / (cb - ca)
        return INTERIOR, a, b, w
    if i == n:
        if P <= ground:
            return LOWEST_HALF_LAYER, n - 1, n - 1, None
        return (BELOW_GROUND, n - 1, n - 1, None) if outside == NEAREST else (BELOW_GROUND, None, None, None)
    return (ABOVE_TOP, 0, 0, None) if outside == NEAREST else (ABOVE_TOP, None, None, None)


def element(column, a, b, w) -> np.float64:
    """y of one (point, variable, target) before the rounding to the stack's type: ``column`` is the variable's n rows."""
    if a is None:
        return np.float64(np.nan)
    if a == b:
        return np.float64(column[a])
    xa, xb = np.float64(column[a]), np.float64(column[b])
    with np.errstate(all="ignore"):
        return xa + w * (xb - xa)


def restate(case: LevelsCase, coordinate=LINEAR, outside=NEAREST, defect=None, rounded=True) -> np.ndarray:
    """``[n_pts, n_var, n_tgt]`` in the case's type (``rounded=False``: the float64 values before the store)."""
    out = np.empty((case.n_pts, case.n_var, case.n_tgt), dtype=np.float64)
    for p in range(case.n_pts):
        pf, ground, s = full_levels(case, p, defect)
        for t in range(case.n_tgt):
            _, a, b, w = bracket(pf, ground, s, case.targets[t], coordinate, outside, defect)
            for v in range(case.n_var):
                column = case.x[p, v, ::-1] if defect == "bottom-first" else case.x[p, v]
                out[p, v, t] = element(column, a, b, w)
    if not rounded:
        return out
    with np.errstate(all="ignore"):
        return out.astype(case.T)


def classes(case: LevelsCase, outside=NEAREST) -> np.ndarray:
    """``[n_pts, n_tgt]`` of class names."""
    out = np.empty((case.n_pts, case.n_tgt), dtype=object)
    for p in range(case.n_pts):
        pf, ground, s = full_levels(case, p)
        for t in range(case.n_tgt):
            out[p, t] = bracket(pf, ground, s, case.targets[t], LINEAR, outside)[0]
    return out


# ---- the same statement, exact -----------------------------------------------------------------------------------------------------
def exact(case: LevelsCase, coordinate=LINEAR) -> tuple[np.ndarray, np.ndarray]:
    """``(value, unit)``, both ``[n_pts, n_var, n_tgt]`` object arrays, for the INTERIOR elements with a finite bracket (None elsewhere):
    the statement evaluated with mpmath from the same inputs — the bracket is the statement's own float64 count, everything after it is
    exact — and one ulp of max(|x[a]|, |x[b]|) in the case's type: the unit errors are measured in (y itself can cancel to zero)."""
    mp = mpmath.mpf
    value = np.full((case.n_pts, case.n_var, case.n_tgt), None, dtype=object)
    unit = np.full((case.n_pts, case.n_var, case.n_tgt), None, dtype=object)
    levels = case.levels()
    for p in range(case.n_pts):
        pf, ground, s = full_levels(case, p)
        if s != s:
            continue
        es = mp(float(s))

        def half(j):
            return mp(float(case.A[j])) + mp(float(case.B[j])) * es

        for t in range(case.n_tgt):
            kind, a, b, _ = bracket(pf, ground, s, case.targets[t], LINEAR, NEAREST)
            if kind != INTERIOR:
                continue
            pa, pb, P = (half(levels[a]) + half(levels[a] + 1)) / 2, (half(levels[b]) + half(levels[b] + 1)) / 2, mp(float(case.targets[t]))
            if coordinate == LOG:
                if not (pa > 0 and pb > 0 and P > 0):
                    continue
                pa, pb, P = mpmath.log(pa), mpmath.log(pb), mpmath.log(P)
            if pa == pb:
                continue
            w = (P - pa) / (pb - pa)
            for v in range(case.n_var):
                xa, xb = float(case.x[p, v, a]), float(case.x[p, v, b])
                if not (math.isfinite(xa) and math.isfinite(xb)) or max(abs(xa), abs(xb)) == 0.0:
                    continue
                value[p, v, t] = mp(xa) + w * (mp(xb) - mp(xa))
                unit[p, v, t] = X.ulp_of(max(abs(xa), abs(xb)), case.T)
    return value, unit


def errors(got: np.ndarray, value: np.ndarray, unit: np.ndarray, scale_to=None) -> np.ndarray:
    """|got - exact| in the units of ``exact`` (NaN where there is no exact value; inf where ``got`` is not finite there)."""
    out = np.full(got.shape, np.nan)
    for idx in np.ndindex(got.shape):
        if value[idx] is None:
            continue
        g = float(got[idx])
        out[idx] = float(abs(mpmath.mpf(g) - value[idx]) / unit[idx]) if math.isfinite(g) else math.inf
    return out


# ---- the comparisons of the GPU test (plain functions: the host test drives them with planted defects) ------------------------------
assert_same_bits = functools.partial(_assert_same_bits, axes="(point, variable, target)")


def check_linear(compute, cases) -> None:
    """``compute(case, coordinate, outside)`` against the restatement, bit for bit, for both policies."""
    for case in cases:
        for outside in (NEAREST, MISSING):
            assert_same_bits(compute(case, LINEAR, outside), reference(case, LINEAR, outside), f"{case.name} linear {outside}")


def log_budget(case: LevelsCase) -> tuple[float, float]:
    """``(bound, numpy's worst)`` in ulps of max(|x[a]|, |x[b]|) of the case's type.  float64: twice numpy's own worst error on the same
    inputs plus SLACK — kernel and numpy evaluate the same statements in the same order with IEEE operations, the one primitive that differs
    is the logarithm (atx_log is budgeted at 1 ulp, glibc's is at about half that), so the kernel may carry up to twice numpy's share.
    float32: the float64 arithmetic under that bound (one float64 ulp is 2^-29 float32 ulps) and one rounding at the store, 0.5 ulp of y,
    which is at most 0.5 ulp of max(|x[a]|, |x[b]|) wherever w is inside [0, 1]."""
    key = (case.name, np.dtype(case.T).name, "numpy-worst")
    if key not in _REFERENCES:
        value, unit = exact_reference(case, LOG)
        y64 = reference(case, LOG, NEAREST, rounded=False)
        if case.T is np.float32:
            unit64 = np.vectorize(lambda u: None if u is None else u * mpmath.ldexp(1, -29), otypes=[object])(unit)
        else:
            unit64 = unit
        e = errors(y64, value, unit64)
        _REFERENCES[key] = float(np.nanmax(e)) if np.isfinite(e).any() else 0.0
    worst = _REFERENCES[key]
    if case.T is np.float32:
        return 0.5 + (2.0 * worst + SLACK) * 2.0**-29, worst
    return 2.0 * worst + SLACK, worst


def check_log(compute, cases, report=None) -> None:
    """``compute(case, "log", outside)``: NaN and infinities where the restatement has them, a level's own bits for a target on a full
    level, and every finite interior value within ``log_budget`` of the exact statement."""
    for case in cases:
        want = reference(case, LOG, NEAREST)
        got = compute(case, LOG, NEAREST)
        what = f"{case.name} log"
        assert got.dtype == want.dtype and got.shape == want.shape
        assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN positions differ"
        inf = np.isinf(want)
        assert np.array_equal(got[inf], want[inf]), f"{what}: infinities differ"
        # the elements the statement copies (outside, the lowest half layer) and the targets on a full level (w == 0): the same bits
        value, unit = exact_reference(case, LOG)
        copied = np.vectorize(lambda v: v is None, otypes=[bool])(value) & ~np.isnan(want)
        assert_same_bits(np.where(copied, got, 0).astype(got.dtype), np.where(copied, want, 0).astype(got.dtype), what + " (copies)")
        on_level = on_a_full_level(case)
        if on_level.any():
            sel = np.broadcast_to(on_level[:, None, :], got.shape) & ~np.isnan(want)
            assert_same_bits(np.where(sel, got, 0).astype(got.dtype), np.where(sel, want, 0).astype(got.dtype), what + " (targets on a full level)")
        e = errors(got, value, unit)
        bound, numpy_worst = log_budget(case)
        worst = float(np.nanmax(e)) if (~np.isnan(e)).any() else 0.0
        if report is not None:
            report[case.name] = dict(kernel=worst, numpy_float64=numpy_worst, bound=bound)
        assert worst <= bound, f"{what}: {worst:.4f} ulps of max(|x[a]|, |x[b]|) from exact > {bound:.4f} (numpy's float64 arithmetic: {numpy_worst:.4f})"


def on_a_full_level(case: LevelsCase) -> np.ndarray:
    """``[n_pts, n_tgt]``: the target equals one of the point's p_full bit for bit (and the point's sp is a number)."""
    out = np.zeros((case.n_pts, case.n_tgt), dtype=bool)
    for p in range(case.n_pts):
        pf, _, s = full_levels(case, p)
        if s == s:
            out[p] = np.isin(case.targets, np.array(pf[:-1], dtype=np.float64))  # (on the lowest level the result is a copy anyway)
    return out


def edge_cases(T) -> list:
    """The cases every class and every planted defect shows in: the base case, a subset column with a level index, a table cut off
    above the ground, and columns that are not monotone.  The host test runs the comparisons on these with each defect planted; the GPU
    test runs them on the kernel."""
    return [base_case(T), shape_case(T, 65, 17, 13, 3, "subset"), shape_case(T, 65, 17, 13, 3, "cut"), shape_case(T, 65, 17, 13, 3, "bent")]


def log_cases(T) -> list:
    """The cases the log coordinate is held to exact arithmetic on: those whose columns are monotone, so that every interior w is inside
    [0, 1] (up to its rounding) and y inside its bracket — what the float32 rule of ``log_budget`` rests on.  The bent columns are held
    to the restatement's bits in the linear coordinate, and in "log" every storage route to the others'."""
    return edge_cases(T)[:3]


# (n_pts, n_lev, n_tgt, n_var): every n_pts of {0, 1, 63, 64, 65, 257}, n_lev of {1, 2, 3, 17, 137}, n_tgt of {1, 13, 64, 65, 129} and n_var of
# {1, 3} at least once, the large ones once each
SHAPES = ((0, 3, 13, 1), (1, 1, 1, 1), (63, 2, 13, 3), (64, 3, 64, 1), (65, 17, 65, 3), (257, 137, 13, 3), (64, 137, 129, 1), (257, 17, 1, 1))


# references are computed once per case and shared; nothing changes them
_REFERENCES: dict = {}


def reference(case: LevelsCase, coordinate, outside, rounded=True) -> np.ndarray:
    key = (case.name, np.dtype(case.T).name, coordinate, outside, rounded)
    if key not in _REFERENCES:
        _REFERENCES[key] = restate(case, coordinate, outside, rounded=rounded)
        _REFERENCES[key].setflags(write=False)
    return _REFERENCES[key]


def exact_reference(case: LevelsCase, coordinate):
    key = (case.name, np.dtype(case.T).name, coordinate, "exact")
    if key not in _REFERENCES:
        _REFERENCES[key] = exact(case, coordinate)
    return _REFERENCES[key]


# ---- cases -----------------------------------------------------------------------------------------------------------------------
def plant_specials(x: np.ndarray) -> None:
    """NaN and +-inf in a few columns: at the top, at the bottom and (columns long enough) in between."""
    n_pts, n_var, n_lev = x.shape
    if n_pts > 1:
        x[1, 0, n_lev // 2] = np.nan
    if n_pts > 2:
        x[2, :, 0] = np.inf
    if n_pts > 3:
        x[3, n_var - 1, n_lev - 1] = -np.inf
    if n_pts > 5 and n_lev > 4:
        x[5, 0, 1], x[5, 0, n_lev - 2] = -np.inf, np.nan
    if n_pts > 6:
        x[6, 0, :] = np.nan
    if n_pts > 7:
        x[7, 0, 0] = -0.0


@functools.lru_cache(maxsize=None)
def base_case(T, specials=True) -> LevelsCase:
    """The fixed case of the GPU test: 17 levels, 257 points with sp uniform in [50 000, 105 000] Pa, the ten BASE_TARGETS — and, added
    behind them, targets equal to a p_full of some point, twice the first of them (a duplicate), in an order that is not sorted."""
    rng = np.random.default_rng(BASE_SEED)
    A, B = eta_table(18)
    sp = rng.uniform(50000.0, 105000.0, 257).astype(T)
    x = (250.0 + 30.0 * rng.standard_normal((257, 3, 17))).astype(T)
    if specials:
        plant_specials(x)
    case = LevelsCase(f"base-{np.dtype(T).name}" + ("" if specials else "-finite"), T, A, B, None, sp, x, np.array(BASE_TARGETS))
    on_level = [full_levels(case, p)[0][k] for p, k in ((0, 0), (10, 5), (64, 16), (200, 9), (256, 15))]
    case.targets = np.array(list(BASE_TARGETS) + [float(v) for v in on_level] + [float(on_level[1])], dtype=np.float64)
    if specials:
        case.sp[4] = np.nan
    return case


def base_class_shares(T) -> dict:
    """The share of each class among the outputs of the ten BASE_TARGETS (a NaN sp aside)."""
    case = base_case(T, specials=False)
    kinds = classes(case)[:, : len(BASE_TARGETS)]
    return {c: float((kinds == c).mean()) for c in CLASSES}


@functools.lru_cache(maxsize=None)
def shape_case(T, n_pts: int, n_lev: int, n_tgt: int, n_var: int, kind: str = "whole") -> LevelsCase:
    """A random case of the given shape.  ``kind``: "whole" (every model level present), "subset" (the rows are levels of a table 7
    longer, with a gap, given by a level index), "cut" (a table cut off above the ground: A[H - 1] != 0) or "bent" (p_full decreases
    towards the ground in the columns with a low sp).  Targets unsorted, with a
    duplicate, one of them on a full level of the first point; NaN and +-inf in the columns; a NaN sp."""
    rng = np.random.default_rng([n_pts, n_lev, n_tgt, n_var, {"whole": 0, "subset": 1, "cut": 2, "bent": 3}[kind], np.dtype(T).itemsize])
    m = None
    if kind == "subset":
        A, B = eta_table(n_lev + 8)
        m = np.array([k + 3 + (k >= n_lev // 2) for k in range(n_lev)])
    elif kind == "cut":
        A, B = eta_table(n_lev + 1, of=n_lev + 3)
    elif kind == "bent":
        A, B = eta_table(n_lev + 1, bend=150000.0)
    else:
        A, B = eta_table(n_lev + 1)
    sp = rng.uniform(50000.0, 105000.0, n_pts).astype(T)
    x = (250.0 + 30.0 * rng.standard_normal((n_pts, n_var, n_lev))).astype(T)
    plant_specials(x)
    targets = np.exp(rng.uniform(np.log(20.0), np.log(115000.0), n_tgt))
    case = LevelsCase(f"{kind}-{n_pts}x{n_var}x{n_lev}-to-{n_tgt}-{np.dtype(T).name}", T, A, B, m, sp, x, targets)
    if n_pts > 0 and n_tgt > 2:
        targets[1] = float(full_levels(case, 0)[0][n_lev // 2])
        targets[n_tgt - 1] = targets[0]
    if n_pts > 8:
        case.sp[8] = np.nan
    return case
