"""The statement of include/atx_search.h twice — a plain float64 loop in numpy, one operation at a time, and a crossing's result in
``fractions.Fraction`` on the same rounded inputs, which is exact — and the cases that tests/test_search_host.py and
tests/test_gpu_search.py share.  It shares no code with the package."""

from __future__ import annotations

import functools
from fractions import Fraction

import numpy as np

import column_tile_restatement as ctr

FORWARD, BACKWARD = "forward", "backward"
UP, DOWN, ANY, MAX, MIN = "up", "down", "any", "max", "min"
CROSSINGS, EXTREMA = (UP, DOWN, ANY), (MAX, MIN)
ULPS_F64 = 11.0  # ATX_SEARCH_ULPS_F64: the header derives it from the statement's six roundings
ONE, SHORT, RAGGED = "one", "tile-1", "tile+tail"  # n_pts: 1, one short of a tile, a tile and fewer points than share a wave
# (points, n_lev, n_var, level_values, n_tgt): the ballot word and its edges, the packed short columns, the limit
SHAPES = [(ONE, 1, 1, False, 1), (SHORT, 2, 1, False, 3), (RAGGED, 3, 0, True, 3), (RAGGED, 13, 4, True, 3), (SHORT, 63, 1, False, 1),
          (RAGGED, 64, 4, False, 3), (ONE, 65, 1, True, 1), (RAGGED, 137, 1, False, 3), (SHORT, 256, 0, True, 1)]
TARGETS = [3.5, np.nan, 4.25]  # (n_tgt == 1: the first)
PLANTED = 13  # points 0 .. 12 of a case with more than 16 points are written by hand (``case``); the rest is random


def bound(T) -> float:
    """In ulps of max(|x[a]|, |x[b]|) in the type ``T``: a float64 ulp is 2^-29 float32 ulps, and float32 adds its one rounding."""
    return ULPS_F64 if T is np.float64 else 0.5 + ULPS_F64 * 2.0**-29


def tile(dtype: str, shape: tuple) -> int:
    """The points of a tile of the column kernel for the shape on the 16-byte route (``search_carve`` of csrc/search/atx_search.hip)."""
    _, n_lev, n_var, has_lv, n_tgt = shape
    elem, V = np.dtype(dtype).itemsize, ctr.vec(dtype)
    x_pitch, s_pitch = -(-n_var * n_lev // V) * V, -(-n_lev // V) * V
    per_point = (n_var + has_lv) * n_tgt
    r = ctr.round16
    return ctr.tile_points(lambda pt: r(pt * x_pitch * elem) + r(pt * s_pitch * elem) + r(pt * per_point * elem) + (r(n_lev * 8) if has_lv else 0)
                           + 2 * r(pt * n_tgt * 8))[0]


def points(dtype: str, shape: tuple) -> int:
    kind, n_lev = shape[0], shape[1]
    packed = max(1, 64 // (1 << max(n_lev - 1, 0).bit_length()))  # the (point, target) pairs that share a wave
    return {ONE: 1, SHORT: tile(dtype, shape) - 1, RAGGED: tile(dtype, shape) + max(1, packed - 1)}[kind]


def crosses(mode: str, here: np.ndarray, following: np.ndarray, T: np.float64) -> np.ndarray:
    up, down = (here <= T) & (T < following), (here >= T) & (T > following)
    return up if mode == UP else down if mode == DOWN else up | down


def statement(s, x, targets, direction, mode, level_values=None):
    """``s [n_pts, n_lev]``, ``x [n_pts, n_var, n_lev]`` in the storage type, ``level_values`` float64 ``[n_lev]`` or None.  Returns
    ``(y [n_pts, n_var (+ 1), n_tgt]`` in that type, ``count`` uint8 ``[n_pts, n_tgt]``, ``{(p, t): (T, a, b)}``: the target and the rows
    in memory of every crossing).  An extremum has one target, whatever ``targets`` holds."""
    n_pts, n_var, n = x.shape
    n_tgt = 1 if mode in EXTREMA else len(targets)
    rows = np.arange(n) if direction == FORWARD else np.arange(n)[::-1]  # e[k] = s[rows[k]]
    y = np.full((n_pts, n_var + (level_values is not None), n_tgt), np.nan, dtype=x.dtype)
    count, crossing = np.zeros((n_pts, n_tgt), dtype=np.uint8), {}

    def columns(p, row):  # every variable's value on a row, float64
        values = x[p, :, row].astype(np.float64)
        return values if level_values is None else np.append(values, np.float64(level_values[row]))

    with np.errstate(all="ignore"):
        for p in range(n_pts):
            e = s[p].astype(np.float64)[rows]
            if mode in EXTREMA:
                held = e[~np.isnan(e)]
                if held.size:
                    extremum = held.max() if mode == MAX else held.min()
                    equal = np.flatnonzero(e == extremum)
                    y[p, :, 0] = columns(p, rows[equal[0]]).astype(x.dtype)
                    count[p, 0] = min(equal.size, 255)
                continue
            for t, g in enumerate(targets):
                T = np.float64(g)
                steps = np.flatnonzero(crosses(mode, e[:-1], e[1:], T))
                count[p, t] = min(steps.size, 255)
                if steps.size:
                    k = steps[0]
                    a, b = rows[k], rows[k + 1]
                    w = (T - e[k]) / (e[k + 1] - e[k])
                    xa, xb = columns(p, a), columns(p, b)
                    d = xb - xa
                    q = w * d
                    y[p, :, t] = (xa + q).astype(x.dtype)
                    crossing[(p, t)] = (T, a, b)
                elif e[n - 1] == T:
                    y[p, :, t] = columns(p, rows[n - 1]).astype(x.dtype)
    return y, count, crossing


def worst_ulps(got, s, x, crossing, level_values=None) -> float:
    """The largest distance of ``got`` from the exact statement over the crossings with finite ends, in ulps of max(|x[a]|, |x[b]|) in
    the type of ``got``."""
    worst = 0.0
    for (p, t), (T, a, b) in crossing.items():
        if not (np.isfinite(s[p, a]) and np.isfinite(s[p, b])):
            continue
        w = (Fraction(float(T)) - Fraction(float(s[p, a]))) / (Fraction(float(s[p, b])) - Fraction(float(s[p, a])))
        for v in range(got.shape[1]):
            xa, xb = (x[p, v, a], x[p, v, b]) if v < x.shape[1] else (level_values[a], level_values[b])
            if np.isfinite(xa) and np.isfinite(xb) and max(abs(xa), abs(xb)) > 0:
                exact = Fraction(float(xa)) + w * (Fraction(float(xb)) - Fraction(float(xa)))
                scale = np.spacing(got.dtype.type(max(abs(xa), abs(xb))))
                worst = max(worst, float(abs(Fraction(float(got[p, v, t])) - exact) / Fraction(float(scale))))
    return worst


@functools.lru_cache(maxsize=None)
def case(dtype: str, shape: tuple):
    """``(s, x, targets, level_values)`` of a shape.  The random part: whole numbers 0 .. 7 — plateaus, turns and targets ON levels are
    common — every other point stretched by an odd factor, and every sixth point lifted far above every target, so that the
    statement alone has pairs without a crossing, with one and with several at every n_lev >= 3 (tests/test_search_host.py checks the
    shares).  The targets: between the levels, NaN, and between other levels.  With more than 16 points, points 0 .. 12 are by hand, with
    T = targets[0], lo = T - 2, hi = T + 2 (each as far as n_lev allows): 0 no crossing; 1 a crossing at the first step; 2 at the last;
    3 the target ON the first level; 4 on an interior level; 5 on the last level alone; 6 a plateau at the target; 7 three crossings of
    alternating sense; 8 / 9 a run of NaN at either end of the column (the scan's start in one direction: pressure levels under the
    ground); 10 all NaN; 11 both infinities; 12 two equal maxima and two equal minima."""
    T = np.dtype(dtype).type
    _, n_lev, n_var, has_lv, n_tgt = shape
    n_pts, n = points(dtype, shape), n_lev
    rng = np.random.default_rng(100 * n_lev + 10 * n_var + n_tgt)
    s = rng.integers(0, 8, (n_pts, n)).astype(np.float64)
    s[1::2] *= 1.0137
    s[5::6] += 1000.0
    targets = np.array(TARGETS[:n_tgt])
    g, lo, hi = targets[0], targets[0] - 2.0, targets[0] + 2.0
    if n_pts > 16:
        s[0] = lo
        s[1], s[2] = hi, lo
        s[1, 0], s[2, n - 1] = lo, hi
        s[3], s[4], s[5], s[6] = hi, hi, lo, hi
        s[3, 0], s[4, : n // 2], s[4, n // 2], s[5, n - 1], s[6, 0], s[6, 1:4] = g, lo, g, g, lo, g
        s[7] = hi
        s[7, 0:3:2] = lo
        s[8, :2], s[9, -2:], s[10] = np.nan, np.nan, np.nan
        s[11, 1 % n], s[11, n - 1 - 1 % n] = np.inf, -np.inf
        s[12, [1 % n, n - 1 - 1 % n]], s[12, [2 % n, n - 1 - 2 % n]] = 9.0, -9.0
    x = (30.0 * rng.standard_normal((n_pts, n_var, n)) + 250.0).astype(T)
    if n_var:
        x[n_pts // 2, 0, n // 2] = np.nan
    level_values = np.cumsum(rng.uniform(1.0, 90.0, n)) if has_lv else None
    return s.astype(T), x, targets, level_values


@functools.lru_cache(maxsize=None)
def reference(dtype: str, shape: tuple, direction: str, mode: str):
    """The numpy statement on the case, computed once for every test that asks."""
    s, x, targets, level_values = case(dtype, shape)
    return statement(s, x, targets, direction, mode, level_values)
