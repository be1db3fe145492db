"""The statement of include/atx_coord.h twice — a plain float64 loop in numpy, one operation at a time, and the same statement in
``fractions.Fraction`` on the same rounded inputs, which is exact — and the cases that tests/test_coord_host.py and tests/test_gpu_coord.py
share.  It shares no code with the package."""

from __future__ import annotations

import functools
from fractions import Fraction

import numpy as np

NEAREST, MISSING = "nearest", "missing"
ULPS_F64 = 11.0  # ATX_COORD_ULPS_F64: the header derives it from the statement's six roundings
SHAPES = [(1, 1, 1, 1), (257, 2, 1, 3), (700, 13, 3, 5), (300, 37, 2, 13), (70, 256, 1, 4)]  # (n_pts, n_lev, n_var, n_tgt)


def bound(T) -> float:
    """In ulps of max(|x[a]|, |x[b]|) in the type ``T``: a float64 ulp is 2^-29 float32 ulps, and float32 adds its one rounding."""
    return ULPS_F64 if T is np.float64 else 0.5 + ULPS_F64 * 2.0**-29


def usable(c: np.ndarray) -> bool:
    if len(c) == 1:
        return bool(c[0] == c[0])
    return bool((c[1:] > c[:-1]).all() or (c[1:] < c[:-1]).all())


def statement(c, x, targets, offset=None, floor=None, outside=NEAREST):
    """``c [n_pts, n_lev]``, ``x [n_pts, n_var, n_lev]`` in the storage type.  Returns ``(y [n_pts, n_var, n_tgt]`` in that type, ``bad``
    uint8 ``[n_pts]``, ``{(p, t): (T, a, b)}``: the target and the rows in memory of every interior bracket)."""
    n_pts, n_var, n = x.shape
    y = np.full((n_pts, n_var, len(targets)), np.nan, dtype=x.dtype)
    bad, interior = np.zeros(n_pts, dtype=np.uint8), {}
    with np.errstate(all="ignore"):
        for p in range(n_pts):
            cp = c[p].astype(np.float64)
            if not usable(cp):
                bad[p] = 1
                continue
            rows = np.arange(n) if n == 1 or cp[1] > cp[0] else np.arange(n)[::-1]  # e[j] = c[rows[j]]
            e = cp[rows]
            for t, g in enumerate(targets):
                T = np.float64(g) if offset is None else np.float64(g) + np.float64(offset[p])
                if floor is not None and T < np.float64(floor[p]):
                    continue
                i = int(np.count_nonzero(e <= T))
                if 0 < i < n:
                    a, b = rows[i - 1], rows[i]
                    w = (T - e[i - 1]) / (e[i] - e[i - 1])
                    xa, xb = x[p, :, a].astype(np.float64), x[p, :, b].astype(np.float64)
                    d = xb - xa
                    s = w * d
                    y[p, :, t] = (xa + s).astype(x.dtype)
                    interior[(p, t)] = (T, a, b)
                elif i == n and (T == e[n - 1] or outside == NEAREST):
                    y[p, :, t] = x[p, :, rows[n - 1]]
                elif i == 0 and outside == NEAREST:
                    y[p, :, t] = x[p, :, rows[0]]
    return y, bad, interior


def worst_ulps(got, c, x, interior) -> float:
    """The largest distance of ``got`` from the exact statement over the interior brackets with finite ends, in ulps of
    max(|x[a]|, |x[b]|) in the type of ``got``."""
    worst = 0.0
    for (p, t), (T, a, b) in interior.items():
        w = (Fraction(float(T)) - Fraction(float(c[p, a]))) / (Fraction(float(c[p, b])) - Fraction(float(c[p, a])))
        for v in range(x.shape[1]):
            xa, xb = x[p, v, a], x[p, v, b]
            if np.isfinite(xa) and np.isfinite(xb) and max(abs(xa), abs(xb)) > 0:
                exact = Fraction(float(xa)) + w * (Fraction(float(xb)) - Fraction(float(xa)))
                worst = max(worst, float(abs(Fraction(float(got[p, v, t])) - exact) / Fraction(float(np.spacing(max(abs(xa), abs(xb)))))))
    return worst


@functools.lru_cache(maxsize=None)
def case(dtype: str, shape: tuple, extras: bool):
    """``(c, x, targets, offset, floor, planted)`` of a shape: every other point's column integer-valued (targets then fall ON levels),
    the rest stretched by an odd factor; the direction per point at random; about one point in sixteen unusable, the kinds in turn;
    targets outside both ends, duplicated and NaN; ``extras``: an integer-valued offset and a floor inside the column, a NaN in each."""
    T = np.dtype(dtype).type
    n_pts, n_lev, n_var, n_tgt = shape
    rng = np.random.default_rng(1000 * n_lev + n_tgt + (7 if extras else 0))
    c = rng.integers(-3, 4, (n_pts, 1)) + np.cumsum(rng.integers(1, 5, (n_pts, n_lev)), axis=1).astype(np.float64)
    c[1::2] *= 1.0137
    down = rng.random(n_pts) < 0.5
    c[down] = c[down, ::-1]
    c = c.astype(T)
    kinds = ["nan"] + (["equal"] if n_lev >= 2 else []) + (["turn"] if n_lev >= 3 else [])
    planted = {}
    for j, p in enumerate(range(5, n_pts, 16)):
        kind, k = kinds[j % len(kinds)], int(rng.integers(0, max(1, n_lev - 2)))
        planted[p] = kind
        if kind == "nan":
            c[p, k] = np.nan
        elif kind == "equal":
            c[p, k + 1] = c[p, k]
        else:
            c[p, k + 1] = c[p, k] + (c[p, k] - c[p, k + 2])  # beyond c[k] on the far side of c[k + 2]: one step turns
    x = (30.0 * rng.standard_normal((n_pts, n_var, n_lev)) + 250.0).astype(T)
    x[n_pts // 2, 0, n_lev // 2] = np.nan
    top = 2.5 * n_lev
    fixed = [float(int(top / 2)), -1.0e6, 1.0e6, float(int(top / 2)), np.nan, 2.0]
    targets = np.array((fixed + list(np.round(rng.uniform(-2.0, top + 2.0, n_tgt) * 4) / 4))[:n_tgt] if n_tgt > 1 else [3.0])
    offset = floor = None
    if extras:
        offset, floor = rng.integers(-2, 3, n_pts).astype(T), rng.uniform(0.0, 0.75 * top, n_pts).astype(T)
        offset[n_pts // 3], floor[n_pts // 4] = np.nan, np.nan
    return c, x, targets, offset, floor, planted


@functools.lru_cache(maxsize=None)
def reference(dtype: str, shape: tuple, extras: bool, outside: str):
    """The numpy statement on the case, computed once for every test that asks."""
    c, x, targets, offset, floor, _ = case(dtype, shape, extras)
    return statement(c, x, targets, offset, floor, outside)
