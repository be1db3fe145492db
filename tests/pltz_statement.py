"""The statement of ``atx_pltz_interpolate`` (include/atx_pltz.h) restated, and the cases the host and the GPU test share.  It shares no code
with the package; the hydrostatic integral c[k] comes from ``geopotential_restatement`` (``column`` in numpy float64, ``exact`` in mpmath).

``outputs`` is the statement after c[k] in the header's order, run twice: over numpy float64 scalars (one IEEE operation per Python
operation), where every comparison is recorded, and over mpmath at 240 bits (``gr.exact``'s precision, >= 50 digits), where the record —
branches and brackets — is replayed.  The host test asserts that every decision of every case has a margin: the replayed ones are exact.

Errors are in ulps of the case's type: of |y| for t and msl; for z of max(|zs|, max_k |c[k]|) of the point, the magnitude the sum passes
through.  The rule is ``levels_restatement.log_budget``'s: float64 within twice numpy's own pinned worst error of the class plus 2 ulps;
float32 0.5 ulp (the store) plus that float64 bound scaled by 2^-29.
"""

from __future__ import annotations

import functools
import math

import mpmath
import numpy as np

import geopotential_restatement as gr
from hybrid_column_common import eta_table

G, GAMMA, RD = 9.80665, 0.0065, gr.RD
LINEAR, LOG = "linear", "log"
WHOLE, LOWEST_17_OF_25 = "whole", "lowest-17-of-25"
SHAPES = ((65, 1, WHOLE), (257, 2, WHOLE), (257, 17, LOWEST_17_OF_25), (65, 137, WHOLE))
LEVELS_HPA = (1, 10, 50, 100, 250, 400, 500, 700, 850, 925, 1000, 1050, 1080)
THRESHOLDS = dict(hgt=(2000.0, 2500.0), tstar=(290.5,), t0=(290.5, 298.0), tz=(255.0,), zs=(0.001,))
MARGIN = 1e-9
SLACK = 2.0
# one block per branch: (hgt in m, T* in K); None: |zs| < 0.001.  Then the three NaN blocks.
BLOCKS = ((500.0, 280.0), (2200.0, 270.0), (3000.0, 270.0), (3000.0, 300.0), (1000.0, 288.0), (300.0, 295.0), (1500.0, 240.0), (None, 285.0),
          (-100.0, 289.0))
NAN_SP, NAN_ZS, NAN_T = len(BLOCKS), len(BLOCKS) + 1, len(BLOCKS) + 2
N_BLOCKS = len(BLOCKS) + 3


NUMPY = (np.float64, np.log, np.exp)
EXACT = (lambda x: mpmath.mpf(float(x)), mpmath.log, mpmath.exp)


def outputs(arithmetic, geo: gr.GeoCase, p: int, c: list, targets, log: bool, replay=None) -> tuple[list, dict]:
    """``[t at every target, z at every target, msl]`` of point p, and what the margins are measured on with, under "record", what every
    comparison gave; ``c``: c[k] in the arithmetic; ``replay``: the record to take in place of the comparisons."""
    (num, ar_log, ar_exp), n, record, replayed = arithmetic, geo.n_lev, [], iter(replay or ())

    def decide(condition) -> bool:
        record.append(bool(condition) if replay is None else next(replayed))
        return record[-1]

    one, two, L = num(1.0), num(2.0), n - 1
    s, zs = num(geo.sp[p]), num(geo.zs[p])
    half = lambda j: num(geo.A[j]) + num(geo.B[j]) * s  # noqa: E731
    pk = [(half(geo.first + k) + half(geo.first + k + 1)) / two for k in range(n)]
    pg = half(geo.n_half - 1)
    t = [num(v) for v in geo.t[p]]
    g, rd, gamma = num(G), num(RD), num(GAMMA)
    kappa = gamma * rd / g
    coord = ar_log if log else (lambda v: v)
    hgt = zs / g
    tstar = t[L] + (kappa * t[L]) * (pg / pk[L] - one)
    t0 = tstar + gamma * hgt
    alpha, tz = kappa, tstar
    cold, warm = decide(tstar <= 290.5), decide(t0 > 290.5)
    if cold and warm:
        alpha = (rd * (num(290.5) - tstar)) / zs
    if decide(tstar > 290.5) and warm:
        alpha, tz = num(0.0), num(0.5) * (num(290.5) + tstar)
    info = dict(hgt=hgt, tstar=tstar, t0=t0, tz=tz, zs=abs(zs), pk=pk, pg=pg, record=record)
    if decide(tz < 255.0):
        tz = num(0.5) * (num(255.0) + tz)
    nan = num(math.nan)
    if decide(s != s or zs != zs):
        return [nan] * (2 * len(targets) + 1), info
    ts, zz = [], []
    for P in (num(v) for v in targets):
        i = sum(decide(v <= P) for v in pk)
        if i == 0:
            yt = yz = nan
        elif i < n or decide(P <= pg):
            a = i - 1 if i < n else L
            pb, tb, cb = (pk[i], t[i], c[i]) if i < n else (pg, tstar, zs)
            w = (coord(P) - coord(pk[a])) / (coord(pb) - coord(pk[a]))
            yt, yz = t[a] + w * (tb - t[a]), c[a] + w * (cb - c[a])
        elif not decide(P > pg):
            yt = yz = nan
        else:
            l = ar_log(P / pg)
            if decide(hgt < 2000.0):
                y = kappa * l
            else:
                plateau = t0 if decide(t0 < 298.0) else num(298.0)
                t0p = plateau if decide(hgt > 2500.0) else num(0.002) * ((num(2500.0) - hgt) * t0 + (hgt - num(2000.0)) * plateau)
                y = num(0.0) if decide(t0p < tstar) else ((rd * (t0p - tstar)) / zs) * l
            y2 = y * y
            y3 = y2 * y
            yt = tstar * (((one + y) + y2 / two) + y3 / num(6.0))
            y = alpha * l
            yz = zs - ((rd * tz) * l) * ((one + y / two) + (y * y) / num(6.0))
        ts.append(yt)
        zz.append(yz)
    if decide(abs(zs) < 0.001):
        msl = pg
    else:
        x = (alpha * zs) / (rd * tz)
        msl = pg * ar_exp((zs / (rd * tz)) * ((one - x / two) + (x * x) / num(3.0)))
    return ts + zz + [msl], info


@functools.lru_cache(maxsize=None)
def reference(geo_name: str, log: bool):
    """``(numpy float64 [n_pts, rows], exact [n_pts, rows] (None where it is no number), one ulp of the unit [n_pts, rows], infos)`` of a
    case of ``CASES``: computed once, shared, never changed."""
    geo, targets = CASES[geo_name]
    rows = 2 * len(targets) + 1
    want = np.empty((geo.n_pts, rows))
    exact, unit, infos = np.full((geo.n_pts, rows), None, dtype=object), np.full((geo.n_pts, rows), None, dtype=object), []
    c_exact = gr.exact_reference(geo)[0]
    with mpmath.workprec(240), np.errstate(all="ignore"):
        for p in range(geo.n_pts):
            values, info = outputs(NUMPY, geo, p, gr.column(geo, p), targets, log)
            want[p] = values
            infos.append(info)
            cs = [mpmath.nan if v is None else v for v in c_exact[p]]
            numbers = [abs(v) for v in c_exact[p] if v is not None]
            if not numbers or not math.isfinite(float(geo.zs[p])):
                continue
            z_unit = max(numbers + [abs(mpmath.mpf(float(geo.zs[p])))])
            info["z_unit"] = float(z_unit)
            for j, v in enumerate(outputs(EXACT, geo, p, cs, targets, log, info["record"])[0]):
                magnitude = z_unit if len(targets) <= j < 2 * len(targets) else abs(v)
                if mpmath.isfinite(v) and magnitude > 0:
                    exact[p, j], unit[p, j] = v, gr.ulp_of(magnitude, geo.T)
    want.setflags(write=False)
    return want, exact, unit, infos


def worst_errors(got: np.ndarray, geo_name: str, log: bool, unit_scale: float = 1.0) -> dict:
    """The worst |got - exact| per variable, in ulps of the unit times ``unit_scale``."""
    _, exact, unit, _ = reference(geo_name, log)
    e = gr.errors(got, exact, unit, unit_scale)
    n_tgt = (got.shape[1] - 1) // 2
    parts = dict(t=e[:, :n_tgt], z=e[:, n_tgt:2 * n_tgt], msl=e[:, 2 * n_tgt:])
    return {k: float(np.nanmax(v)) if (~np.isnan(v)).any() else 0.0 for k, v in parts.items()}


def numpy_worst(geo_name: str, log: bool) -> dict:
    """numpy's float64 arithmetic against exact, in FLOAT64 ulps whatever the case's type."""
    scale = 2.0**-29 if CASES[geo_name][0].T is np.float32 else 1.0
    return worst_errors(reference(geo_name, log)[0], geo_name, log, scale)


def bound(T, numpy_pinned: float) -> float:
    ceiling = 2.0 * numpy_pinned + SLACK
    return 0.5 + ceiling * 2.0**-29 if T is np.float32 else ceiling


# ---- cases -----------------------------------------------------------------------------------------------------------------------
CASES: dict = {}


def make_case(T, n_pts: int, n_lev: int, table: str = WHOLE, levels_hpa=LEVELS_HPA, seed: int = 0) -> str:
    """Point p belongs to block p % N_BLOCKS.  sp is a little above one of the lower targets, so that this target lies in the lowest
    half layer (whose relative thickness is 0.6 % at 137 levels); t[L] is chosen for the block's T*, +- 1 K, hgt is the block's +- 4 %.
    Returns the name under which ``CASES`` holds ``(GeoCase, targets in Pa)``."""
    name = f"pltz-{table}-{n_pts}x{n_lev}-{np.dtype(T).name}-{seed}" + ("" if levels_hpa is LEVELS_HPA else "-to-" + "-".join(map(str, levels_hpa)))
    if name in CASES:
        return name
    rng = np.random.default_rng([20261126, n_pts, n_lev, table == WHOLE, seed])
    A, B = eta_table(n_lev + 1 if table == WHOLE else 26, bend=40000.0)
    first = len(A) - 1 - n_lev
    targets = np.array(levels_hpa, dtype=np.float64) * 100.0
    # sp is drawn from the lower targets (the largest is under everyone's ground) — those from which the deepest extrapolation,
    # log(P_max / sp), is at most half the depth log(p_g / p[k0]) of what the column sums to a number: k0 = 0, or the level under the NaN
    # of the NaN-t block (which takes the largest candidate otherwise).  Then |z| under the ground stays below the magnitude the
    # hydrostatic sum passes through, the unit of z: the float32 store's half ulp of |z| is at most half an ulp of the unit.
    full = lambda k, s: ((A[first + k] + B[first + k] * s) + (A[first + k + 1] + B[first + k + 1] * s)) / 2.0  # noqa: E731
    shallow = lambda v, k: math.log(targets.max() / v) <= 0.5 * math.log(v / full(k, v))  # noqa: E731
    low = np.array([v * 100.0 for v in LEVELS_HPA if 500 <= v < max(LEVELS_HPA) and shallow(v * 100.0, 0)])
    block = np.arange(n_pts) % N_BLOCKS
    chosen = rng.choice(low, n_pts)
    under_nan = n_lev // 2 + 1
    if under_nan < n_lev:
        chosen[(block == NAN_T) & ~np.array([shallow(v, under_nan) for v in chosen])] = low.max()
    sp = (chosen * (1.0 + 0.003 * rng.uniform(0.2, 1.0, n_pts))).astype(T)
    t = rng.uniform(220.0, 300.0, (n_pts, n_lev)).astype(T)
    q = rng.uniform(0.0, 0.02, (n_pts, n_lev)).astype(T)
    zs = np.empty(n_pts, dtype=T)
    kappa = GAMMA * RD / G
    for p in range(n_pts):
        hgt, tstar = BLOCKS[block[p]] if block[p] < len(BLOCKS) else BLOCKS[0]
        zs[p] = (0.0005, 0.0, -0.0004)[p % 3] if hgt is None else hgt * rng.uniform(0.96, 1.04) * G
        s = np.float64(sp[p])
        pg = A[-1] + B[-1] * s
        p_low = ((A[first + n_lev - 1] + B[first + n_lev - 1] * s) + pg) / 2.0
        t[p, -1] = (tstar + rng.uniform(-1.0, 1.0)) / (1.0 + kappa * (pg / p_low - 1.0))
    sp[block == NAN_SP] = np.nan
    zs[block == NAN_ZS] = np.nan
    t[block == NAN_T, n_lev // 2] = np.nan
    CASES[name] = (gr.GeoCase(name, T, A, B, sp, zs, t, q), targets)
    return name


# the filter tests' cases: 684 points (a 10 degree grid) x 17 levels, one seed per date; "interior": targets inside every point's column
WORLD_LEVELS = dict(filter=(1080, 500, 850, 10, 1000, 300, 1050), interior=(300, 50, 100, 400, 200))
WORLD_SEEDS = (1, 2)


def world_case(T, which: str, seed: int) -> str:
    return make_case(T, 684, 17, WHOLE, WORLD_LEVELS[which], seed)
