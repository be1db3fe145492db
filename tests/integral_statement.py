"""The statement of include/atx_integral.h twice — ONE plain loop, run in numpy float64 (one IEEE operation at a time) and in
``fractions.Fraction`` on the same rounded inputs, which is exact — and the seeded case that tests/test_integral_host.py and
tests/test_gpu_integral.py share.  It shares no code with the package."""

from __future__ import annotations

import functools
import math
from fractions import Fraction

import numpy as np

HYBRID, PRESSURE = "hybrid", "pressure"
SUM, MEAN = "integral", "mean"
BLOCK, G = 8, 9.80665  # ATX_INTEGRAL_BLOCK, ATX_INTEGRAL_G
SHAPES = [(1, 1, 1, 1, 1), (257, 13, 3, 4, 3), (300, 37, 2, 3, 5), (70, 137, 4, 5, 2)]  # (n_pts, n_lev, n_var, n_term, n_bnd)

f64 = np.float64
exact = lambda v: Fraction(float(v))  # noqa: E731


def ulps_f64(n_lev: int, K: float, kind: str) -> float:
    """ATX_INTEGRAL_ULPS_F64 of the header, twice for a mean."""
    return (16.0 * K + BLOCK + (n_lev + BLOCK - 1) // BLOCK + 2) * (2 if kind == MEAN else 1)


def bound(T, n_lev: int, K: float, kind: str) -> float:
    """In ulps of sum |w f| / divisor in ``T``: a float64 ulp is 2^-29 float32 ulps, and float32 adds its one rounding."""
    return ulps_f64(n_lev, K, kind) if T is np.float64 else 0.5 + ulps_f64(n_lev, K, kind) * 2.0**-29


def weights(n, sp, top, bottom, A, B, P, num):
    """``w[0..n-1]`` of one (point, bound) in the arithmetic of ``num``; ``bottom`` may be the float ``inf`` in either."""
    zero, w = num(0.0), []
    if P is None:
        for k in range(n):
            lo, hi = num(A[k]) + num(B[k]) * sp, num(A[k + 1]) + num(B[k + 1]) * sp
            a = lo if lo > top else top
            c = hi if hi < bottom else bottom
            w.append(c - a if c > a else zero)
        return w
    m = sum(1 for k in range(n) if num(P[k]) <= sp)

    def share(pj, pn, lower_end):
        a = pj if pj > top else top
        c = pn if pn < bottom else bottom
        if not c > a:
            return zero
        length, mid = c - a, (a + c) / num(2.0)
        r = (mid - pj) / (pn - pj)
        return length * r if lower_end else length * (num(1.0) - r)

    for k in range(n):
        if k >= m:
            w.append(zero)
            continue
        pk = num(P[k])
        above = share(num(P[k - 1]), pk, True) if k >= 1 else zero
        if k + 1 < m:
            below = share(pk, num(P[k + 1]), False)
        else:
            a = pk if pk > top else top
            c = sp if sp < bottom else bottom
            below = c - a if c > a else zero
        w.append(above + below)
    return w


def reduce(w, x, term, kind, num):
    """``(y, S)``: the blocked sum of one term over one (point, bound) and sum |w f| / divisor; ``None`` where exact arithmetic has no value."""
    v1, v2 = term
    zero = num(0.0)
    acc = wacc = S = zero
    for k0 in range(0, len(w), BLOCK):
        s = ws = zero
        for k in range(k0, min(k0 + BLOCK, len(w))):
            if w[k] != 0:
                f = num(x[v1][k]) if v2 < 0 else num(x[v1][k]) * num(x[v2][k])
                s, ws, S = s + w[k] * f, ws + w[k], S + abs(w[k] * f)
        acc, wacc = acc + s, wacc + ws
    divisor = wacc if kind == MEAN else num(G)
    if num is exact and divisor == 0:
        return None, None
    return acc / divisor, S / divisor


def statement(x, sp, terms, bounds, kind, A=None, B=None, P=None):
    """``x [n_pts, n_var, n_lev]`` and ``sp [n_pts]`` in the storage type -> ``y [n_pts, n_term, n_bnd]`` in that type: the numpy loop."""
    n_pts, _, n = x.shape
    y = np.full((n_pts, len(terms), len(bounds)), np.nan, dtype=x.dtype)
    with np.errstate(all="ignore"):
        for p in range(n_pts):
            s = f64(sp[p])
            if s != s:
                continue
            for b, (top, bottom) in enumerate(bounds):
                w = weights(n, s, f64(top), f64(bottom), A, B, P, f64)
                for t, term in enumerate(terms):
                    y[p, t, b] = reduce(w, x[p], term, kind, f64)[0]
    return y


def worst_ulps(got, x, sp, terms, bounds, kind, A=None, B=None, P=None, points=None):
    """``(worst, worst / bound)`` over the results with a finite exact value: the distance of ``got`` from the statement in exact
    arithmetic in ulps of S in the type of ``got``, and the same as a fraction of the header's bound for that (point, bound) — K is
    max P over the smallest non-zero weight, in either arithmetic."""
    n = x.shape[2]
    T = got.dtype.type
    worst = worst_of_bound = 0.0
    levels = [float(v) for v in P] if P is not None else []
    for p in range(x.shape[0]) if points is None else points:
        if not np.isfinite(sp[p]):
            continue
        for b, (top, bottom) in enumerate(bounds):
            we = weights(n, exact(sp[p]), exact(top), bottom if math.isinf(bottom) else exact(bottom), A, B, P, exact)
            with np.errstate(all="ignore"):
                wf = weights(n, f64(sp[p]), f64(top), f64(bottom), A, B, P, f64)
            nonzero = [float(v) for v in (*we, *wf) if v != 0]
            if not nonzero:
                continue
            halves = [float(A[k] + B[k] * f64(sp[p])) for k in range(n + 1)] if P is None else levels
            K = max([float(sp[p]), float(top), *halves] + ([] if math.isinf(bottom) else [float(bottom)])) / min(nonzero)
            for t, term in enumerate(terms):
                if not np.isfinite(got[p, t, b]):
                    continue
                value, S = reduce(we, x[p], term, kind, exact)
                if value is None or S == 0:
                    continue
                ulps = float(abs(exact(got[p, t, b]) - value) / exact(np.spacing(T(float(S)))))
                worst, worst_of_bound = max(worst, ulps), max(worst_of_bound, ulps / bound(T, n, K, kind))
    return worst, worst_of_bound


def table(n_lev: int):
    """Half levels of a hybrid column: pure pressure (B = 0) above eta = 0.3, the ground (A = 0, B = 1) last."""
    eta = np.arange(n_lev + 1, dtype=np.float64) / n_lev
    return 20000.0 * eta * (1.0 - eta), (np.maximum(eta - 0.3, 0.0) / 0.7) ** 2


@functools.lru_cache(maxsize=None)
def case(dtype: str, shape: tuple, mode: str) -> dict:
    """The seeded case of a shape: ``x``, ``sp``, ``terms``, ``bounds`` and ``A`` / ``B`` or ``P``.  Planted from point 3 on (where the shape
    has them): an sp under P[0], on a level, between two levels, beyond the last level, NaN; NaN in every variable under the ground
    (PRESSURE); a NaN in variable 0 at the top level of point 9.  Bounds: the whole column, one inside a layer or segment, one with
    edges on levels, one wholly under the ground, one ordinary; terms: a variable, a square (v1 == v2), a product, two more."""
    T = np.dtype(dtype).type
    n_pts, n_lev, n_var, n_term, n_bnd = shape
    rng = np.random.default_rng(100 * n_lev + n_bnd + (1 if mode == PRESSURE else 0))
    x = (30.0 * rng.standard_normal((n_pts, n_var, n_lev)) + 10.0).astype(T)
    sp = rng.uniform(50000.0, 104000.0, n_pts).astype(T)
    out = dict(A=None, B=None, P=None)
    if mode == PRESSURE:
        P = out["P"] = np.round(np.linspace(1000.0, 100000.0, n_lev) / 100.0) * 100.0 if n_lev > 1 else np.array([50000.0])
        j = n_lev // 2
        step = P[j] - P[j - 1] if n_lev > 1 else 1000.0
        inside = (P[j - 1] + step / 4, P[j - 1] + step / 2) if n_lev > 1 else (P[0] + 10.0, P[0] + 20.0)
        edges = (P[1], P[-2]) if n_lev >= 4 else (P[0], P[0] + 1000.0)
        if n_pts > 8:
            sp[3:8] = [500.0, P[j], P[j] - 0.25 * step, P[-1] + 3000.0, np.nan]
        for p in range(n_pts):
            x[p, :, int(np.count_nonzero(P <= sp[p])):] = np.nan  # under the ground: must not show
    else:
        A, B = out["A"], out["B"] = table(n_lev)
        last_pure = int(np.flatnonzero(B == 0)[-1])
        inside = (30000.0, 30010.0)
        edges = (A[1], A[last_pure]) if n_lev >= 4 and A[last_pure] > A[1] else (0.0, 50000.0)
        if n_pts > 8:
            sp[7] = np.nan
    if n_pts > 9:
        x[9, 0, 0] = np.nan  # above the ground: must show
    bounds = [(0.0, math.inf), inside, edges, (120000.0, 130000.0), (50000.0, 85000.0)][:n_bnd]
    last = n_var - 1
    terms = [(0, -1), (last, last), (0, 1 % n_var), (last, -1), (1 % n_var, 2 % n_var)][:n_term]
    return dict(x=x, sp=sp, terms=terms, bounds=[(float(a), float(b)) for a, b in bounds], **out)


@functools.lru_cache(maxsize=None)
def reference(dtype: str, shape: tuple, mode: str, kind: str) -> np.ndarray:
    """The numpy statement on the case, computed once for every test that asks."""
    c = case(dtype, shape, mode)
    return statement(c["x"], c["sp"], c["terms"], c["bounds"], kind, c["A"], c["B"], c["P"])
