"""The statement of ``atx_parcel_columns`` (include/atx_parcel.h) written ONCE over an arithmetic — numpy float64 scalars, one IEEE
operation per Python operation, and mpmath at 240 bits — and the small cases that tests/test_parcel_host.py and tests/test_gpu_parcel.py
share.  It shares no code with the package.

``ascent`` returns the five outputs of a point, S (the sum of the absolute areas: the unit of ``cape`` and ``cin``) and every decision
with its relative margin; the mpmath run takes its decisions itself, and the host test asserts that both runs decide alike with a
margin of MARGIN.  The rule of the GPU test is ``levels_restatement.log_budget``'s: float64 within twice numpy's own worst error of the
case plus 2 ulps; float32 0.5 ulp (the store) plus that bound scaled by 2^-29."""

from __future__ import annotations

import functools
import math

import mpmath
import numpy as np

HYBRID, PRESSURE = "hybrid", "pressure"
LOWEST, MOST_UNSTABLE = "lowest", "most-unstable"
OUTPUTS = ("cape", "cin", "plcl", "tlcl", "pstart")
RD, RV, KAPPA, LN1E5, BLOCK, NEWTON_STEPS = 287.0597, 461.5250, 2.0 / 7.0, 11.512925464970229, 8, 10
MARGIN, SLACK = 1e-6, 2.0
N_LEVS = (2, 9, 32, 33, 65, 137)
TOP, DEPTH = 6050.0, 30050.0  # Pa: the cases' p_top (a dry column's LCL lies above it) and most-unstable depth
KINDS = 8  # point i of a case is a column of kind i % KINDS (``case``)
CHECKED = 8  # the points of a case that are held to mpmath: every kind once

NUMPY = (np.float64, np.log, np.exp)
EXACT = (lambda x: mpmath.mpf(float(x)), mpmath.log, mpmath.exp)


def pressures(ar, n, sp, A=None, B=None, P=None):
    num = ar[0]
    if P is not None:
        return [num(v) for v in P]
    half = [num(A[j]) + num(B[j]) * sp for j in range(n + 1)]
    return [(half[k] + half[k + 1]) / num(2.0) for k in range(n)]


def ascent(ar, t, q, sp, parcel, A=None, B=None, P=None, top=TOP, depth=DEPTH, steps=NEWTON_STEPS) -> dict:
    """One point.  ``out``: (cape, cin, plcl, tlcl, pstart) in the arithmetic (NaN: ``math.nan``), ``S``, ``decisions`` [(bool, margin)]."""
    num, ar_log, ar_exp = ar
    n, one, nan, decisions = len(t), num(1.0), math.nan, []
    eps = num(RD) / num(RV)

    def decide(a, b, greater_equal=True) -> bool:
        """a >= b (or a > b), recorded with |a - b| / max(|a|, |b|)."""
        scale = max(abs(a), abs(b))
        decisions.append((bool(a >= b if greater_equal else a > b), float(abs(a - b) / scale) if scale != 0 else math.inf))
        return decisions[-1][0]

    failed = dict(out=[nan] * 5, S=None, decisions=decisions)
    sp = num(sp)
    if sp != sp:
        return failed
    p = pressures(ar, n, sp, A, B, P)
    takes_part = [decide(p[k], num(top)) and (P is None or decide(sp, p[k])) for k in range(n)]
    if not any(takes_part):
        return failed
    kt, kb = takes_part.index(True), n - 1 - takes_part[::-1].index(True)
    T, Q = [num(v) for v in t], [num(v) for v in q]
    if any(T[k] != T[k] or Q[k] != Q[k] for k in range(kt, kb + 1)):
        return failed
    lnp = {k: ar_log(p[k]) for k in range(kt, kb + 1)}

    def ln_theta_e(lnT, TL, r, k):
        return (lnT + (num(0.2854) * (one - num(0.28) * r)) * (num(LN1E5) - lnp[k])) + ((num(3.376) / TL - num(0.00254)) * (num(1000.0) * r)) * (one + num(0.81) * r)

    def start(k):
        r = Q[k] / (one - Q[k])
        e = (p[k] * r) / (eps + r)
        lnT = ar_log(T[k])
        TL = num(2840.0) / ((num(3.5) * lnT - ar_log(e / num(100.0))) - num(4.805)) + num(55.0)
        return r, TL, ln_theta_e(lnT, TL, r, k)

    def virtual(Tk, r):
        return (Tk * (one + r / eps)) / (one + r)

    def saturation(Tk, pk):
        es = num(611.21) * ar_exp((num(17.502) * (Tk - num(273.16))) / (Tk - num(32.19)))
        pe = pk - es
        return (eps * es) / pe, pe

    s = kb
    if parcel == MOST_UNSTABLE:
        floor, best = p[kb] - num(depth), None
        for k in range(kb, kt - 1, -1):  # from the ground: the first wins among equals
            if decide(p[k], floor):
                value = start(k)[2]
                if best is None or value > best:
                    best, s = value, k
        others = [start(k)[2] for k in range(kt, kb + 1) if k != s and p[k] >= floor]
        for value in others:
            decide(best, value, greater_equal=False)
    rs, TL, target = start(s)
    pL = p[s] * ar_exp(num(3.5) * ar_log(TL / T[s]))

    b = {s: num(0.0)}
    for k in range(kt, s):
        Tk = T[s] * ar_exp(num(KAPPA) * ar_log(p[k] / p[s]))
        r = rs
        if not decide(p[k], pL):
            lnh = ar_log(p[k] / num(1222.42))  # es = p / 2 at the cap
            cap = (num(32.19) * lnh - num(4780.84632)) / (lnh - num(17.502))
            for _ in range(steps):
                r, pe = saturation(Tk, p[k])
                F = ln_theta_e(ar_log(Tk), Tk, r, k) - target
                d = Tk - num(32.19)
                dr = (r * (p[k] / pe)) * (num(4217.45694) / (d * d))
                w = (num(1000.0) * r) * (one + num(0.81) * r)
                dF = ((one / Tk - (num(0.079912) * dr) * (num(LN1E5) - lnp[k])) - (num(3.376) / (Tk * Tk)) * w) \
                    + ((num(3.376) / Tk - num(0.00254)) * (num(1000.0) * dr)) * (one + num(1.62) * r)
                Tn = Tk - F / dF
                Tk = Tn if Tn < cap else cap
            r = saturation(Tk, p[k])[0]
        tv_p, tv_e = virtual(Tk, r), virtual(T[k], Q[k] / (one - Q[k]))
        decide(tv_p, tv_e)  # the sign of b
        b[k] = num(RD) * (tv_p - tv_e)

    zero, two = num(0.0), num(2.0)
    pos, neg = {}, {}
    for j in range(kt, s):  # step j: levels j (upper) and j + 1 (lower)
        lo, hi, dl = b[j + 1], b[j], lnp[j + 1] - lnp[j]
        if (lo > 0 and hi < 0) or (lo < 0 and hi > 0):
            f = lo / (lo - hi)
            a_lo, a_hi = ((lo * f) * dl) / two, ((hi * (one - f)) * dl) / two
            pos[j], neg[j] = (a_lo, a_hi) if lo > 0 else (a_hi, a_lo)
        else:
            area = ((lo + hi) / two) * dl
            pos[j], neg[j] = (area, zero) if area > 0 else (zero, area)
    first = max((j for j in pos if pos[j] > 0), default=None)
    cape, cin, S = zero, zero, zero
    for k0 in range((n - 1) // BLOCK * BLOCK, -1, -BLOCK):  # blocks of BLOCK steps aligned to the level index, from the ground up
        bp = bn = zero
        for j in range(min(k0 + BLOCK, n) - 1, k0 - 1, -1):
            if j in pos:
                below = first is not None and (j > first or (j == first and b[j + 1] < 0))
                bp, bn, S = bp + pos[j], bn + (neg[j] if below else zero), S + (pos[j] - neg[j])
        cape, cin = cape + bp, cin + bn
    return dict(out=[cape, cin if first is not None else nan, pL, TL, p[s]], S=S, decisions=decisions, start=s)


# ---- cases -------------------------------------------------------------------------------------------------------------------------
def table(n_lev: int):
    """Half levels of a hybrid column: pure pressure (B = 0) above eta = 0.3, the ground (A = 0, B = 1) last."""
    eta = np.arange(n_lev + 1, dtype=np.float64) / n_lev
    return 20000.0 * eta * (1.0 - eta), (np.maximum(eta - 0.3, 0.0) / 0.7) ** 2


def _es(T):
    return 611.21 * np.exp(17.502 * (T - 273.16) / (T - 32.19))


N_MAX = 1024  # the points a case is cut from: point i is the same column whatever n_pts is


@functools.lru_cache(maxsize=None)
def _columns(dtype: str, n_lev: int, mode: str) -> dict:
    T, n_pts = np.dtype(dtype).type, N_MAX
    rng = np.random.default_rng(1000 * n_lev + (1 if mode == PRESSURE else 0))
    out = dict(A=None, B=None, P=None)
    sp = rng.uniform(96000.0, 103000.0, n_pts)
    sp[5::KINDS] = rng.uniform(70000.0, 90000.0, len(sp[5::KINDS]))
    sp = sp.astype(T)
    if mode == PRESSURE:
        out["P"] = np.round(np.geomspace(5000.0, 95000.0, n_lev) / 100.0) * 100.0 if n_lev > 2 else np.array([70000.0, 90000.0])
        p = np.broadcast_to(out["P"], (n_pts, n_lev))
    else:
        A, B = out["A"], out["B"] = table(n_lev)
        half = A[None, :] + B[None, :] * sp[:, None].astype(np.float64)
        p = (half[:, :-1] + half[:, 1:]) / 2.0
    ground = sp[:, None].astype(np.float64)
    kind = (np.arange(n_pts) % KINDS)[:, None]
    lapse = np.where(kind == 0, 0.10, 0.19) + 0.01 * rng.random((n_pts, 1))  # d ln T / d ln p
    t0 = np.where(kind == 0, 285.0, 301.0) + 3.0 * rng.random((n_pts, 1))
    t = np.maximum(t0 * (p / ground) ** lapse, 205.0 + 5.0 * rng.random((n_pts, n_lev)))
    rh = np.where(kind == 0, 0.2, np.where(kind == 1, 0.9995, 0.8)) * np.clip((p / ground - 0.2) / 0.8, 0.02, 1.0) ** 1.5
    warm = (kind == 4) & (p < ground - 6000.0) & (p > ground - 20000.0)  # 4: the ground layer is cold and dry under it
    t = np.where((kind == 4) & (p >= ground - 6000.0), t - 8.0, t)
    rh = np.where(warm, 0.95, np.where((kind == 4) & ~warm, 0.3 * rh, rh))
    e = rh * _es(t)
    q = 0.622 * e / (p - 0.378 * e)
    q = np.where(kind == 2, 1e-14, q)
    t, q = t.astype(T), q.astype(T)
    for i in range(6, n_pts, KINDS):
        t[i, np.flatnonzero(p[i] < ground[i, 0] - 3000.0)[-1]] = np.nan  # the level next to the ground that is 30 hPa or more above it
    if mode == PRESSURE:
        under = p > ground
        t[under], q[under] = np.nan, np.nan
    return dict(t=t, q=q, sp=sp, **out)


def case(dtype: str, n_lev: int, n_pts: int, mode: str) -> dict:
    """``t``, ``q`` [n_pts, n_lev], ``sp`` and ``A`` / ``B`` or ``P``: the first ``n_pts`` of N_MAX columns.  Point i is of kind i % 8: 0 stable
    and dry; 1 nearly saturated at the ground (the LCL below the second level); 2 so dry that the LCL lies above TOP; 3 and 7
    conditionally unstable (sign changes inside steps); 4 a cold dry ground under a warm moist layer (the most unstable level is not the
    lowest); 5 as 3 with a low sp — on pressure levels the ground lies between two levels, and NaN is stored under it in every column;
    6 a NaN in t inside the ascent."""
    c = _columns(dtype, n_lev, mode)
    return dict(t=c["t"][:n_pts], q=c["q"][:n_pts], sp=c["sp"][:n_pts], A=c["A"], B=c["B"], P=c["P"])


@functools.lru_cache(maxsize=None)
def reference(dtype: str, n_lev: int, n_pts: int, mode: str, parcel: str):
    """``(numpy float64 [n_pts, 5], exact [CHECKED, 5] (None where it is no number), unit [CHECKED, 5], runs, S [n_pts])`` of a case,
    computed once: the unit is one ulp, in the case's type, of S for cape and cin and of |y| for the others; ``runs``: the (numpy,
    mpmath) results of the checked points; S: numpy's sum of the absolute areas of every point (NaN where the point has none)."""
    c, T = case(dtype, n_lev, n_pts, mode), np.dtype(dtype).type
    tables = dict(A=c["A"], B=c["B"], P=c["P"])
    want, S = np.empty((n_pts, 5)), np.full(n_pts, np.nan)
    checked = min(CHECKED, n_pts)
    exact, unit, runs = np.full((checked, 5), None, dtype=object), np.full((checked, 5), None, dtype=object), []
    with mpmath.workprec(240), np.errstate(all="ignore"):
        for i in range(n_pts):
            mine = ascent(NUMPY, c["t"][i], c["q"][i], c["sp"][i], parcel, **tables)
            want[i], S[i] = [float(v) for v in mine["out"]], np.nan if mine["S"] is None else float(mine["S"])
            if i >= checked:
                continue
            true = ascent(EXACT, c["t"][i], c["q"][i], c["sp"][i], parcel, **tables)
            runs.append((mine, true))
            for o, v in enumerate(true["out"]):
                if v == v:
                    size = true["S"] if o < 2 else abs(v)
                    exact[i, o], unit[i, o] = v, mpmath.mpf(float(np.spacing(T(float(size))))) if size != 0 else None
    want.setflags(write=False)
    return want, exact, unit, runs, S


def errors(got: np.ndarray, exact: np.ndarray, unit: np.ndarray, scale: float = 1.0) -> np.ndarray:
    """|got - exact| in units (``scale``: the unit's multiple, 2^-29 for float64 values in float32 ulps); NaN where there is no unit."""
    out = np.full(exact.shape, np.nan)
    for idx in np.ndindex(exact.shape):
        if unit[idx] is not None and math.isfinite(float(got[idx])):
            out[idx] = float(abs(mpmath.mpf(float(got[idx])) - exact[idx]) / (unit[idx] * scale))
    return out


def budget(dtype: str, n_lev: int, n_pts: int, mode: str, parcel: str) -> tuple[np.ndarray, np.ndarray]:
    """``(bound [5], numpy's worst [5])`` per output in ulps of the unit in the case's type."""
    want, exact, unit = reference(dtype, n_lev, n_pts, mode, parcel)[:3]
    f32 = dtype == "float32"
    e = errors(want[: len(exact)], exact, unit, 2.0**-29 if f32 else 1.0)
    worst = np.array([np.nanmax(e[:, o]) if np.isfinite(e[:, o]).any() else 0.0 for o in range(5)])
    return (0.5 + (2.0 * worst + SLACK) * 2.0**-29 if f32 else 2.0 * worst + SLACK), worst
