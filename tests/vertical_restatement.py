"""earthkit-meteo's ``vertical.pressure_at_height_levels`` and the two dewpoint conversions of ``q_to_d_height`` / ``d_to_q_height``,
restated in numpy — TEST INFRASTRUCTURE (``oracle/`` is frozen, so the new statements live here).

R: filters/fields/q_height.py:203-213, :416-426 call ``vertical.pressure_at_height_levels(height, t, q, sp, A, B)`` with its default
``alpha_top="ifs"``; :466-475 and :511-514 call ``thermo.dewpoint_from_specific_humidity`` / ``thermo.specific_humidity_from_dewpoint``.
earthkit-meteo is absent here: these are its published statements as restated, with the moist gas constant written
``R(q) = Rd (1 - q) + Rv q`` (Rd = 287.0597, Rv = 461.5250, the constants of the oracle's epsilon).  The other published form,
``Rd (1 + 0.609133 q)``, moves the reference's 2 m dewpoints by 3e-10 relative: no vector here tells the two apart, and nothing more
is claimed.  What pins the pressure path is the reference's Q2M -> D2M literals at its own rtol 1e-7 (tests/test_height_level_humidity.py):
they rule out the dry gas constant (1.3e-7) and p = sp (1.3e-5).

Levels are ordered top first (the reference orders the fields ``level="ascending"``); ``t``, ``q`` are ``[n_lev, ...]``, ``A``, ``B``
hold the n_lev + 1 half-level coefficients.  Everything is evaluated in float64, whatever the width of the inputs.
"""

from __future__ import annotations

import numpy as np

from oracle import oracle

RD, RV = 287.0597, 461.5250
G = 9.80665
EPS_SPECIFIC = 1.0e-8  # R: q_height.py:25


def pressure_at_model_levels(A, B, sp):
    """``(p_full, p_half, alpha)``; ``alpha_top="ifs"``: alpha[0] = ln 2 (delta[0] = ln(p_half[1] / 0.1) feeds nothing else)."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    sp = np.asarray(sp, dtype=np.float64)
    shape = (-1,) + (1,) * sp.ndim
    p_half = A.reshape(shape) + B.reshape(shape) * sp
    with np.errstate(all="ignore"):
        delta = np.empty_like(p_half[1:])
        delta[0] = np.log(p_half[1] / 0.1)
        delta[1:] = np.log(p_half[2:] / p_half[1:-1])
        alpha = np.empty_like(delta)
        alpha[0] = np.log(2.0)
        alpha[1:] = 1.0 - p_half[1:-1] / (p_half[2:] - p_half[1:-1]) * delta[1:]
        p_full = (p_half[:-1] + p_half[1:]) / 2.0
    return p_full, p_half, alpha


def relative_geopotential_thickness(alpha, t, q):
    """dphi[k] = sum over j = n-1 .. k of alpha[j] R(q_j) t_j: numpy's cumsum over the flipped level axis (bottom level first)."""
    t, q = np.asarray(t, dtype=np.float64), np.asarray(q, dtype=np.float64)
    with np.errstate(all="ignore"):
        r = RD * (1.0 - q) + RV * q
        return np.flip(np.cumsum(np.flip(alpha * r * t, axis=0), axis=0), axis=0)


def pressure_at_height_levels(height, t, q, sp, A, B):
    """The pressure (Pa) at ``height`` metres above the ground, float64 ``[...]`` of ``sp``'s shape."""
    p_full, p_half, alpha = pressure_at_model_levels(A, B, sp)
    dphi = relative_geopotential_thickness(alpha, t, q)
    n = dphi.shape[0]
    tdphi = float(height) * G
    i = (tdphi > dphi).sum(axis=0)
    with np.errstate(all="ignore"):
        below = p_half[n] + tdphi / dphi[n - 1] * (p_full[n - 1] - p_half[n])
        a = n - i - 1
        a = np.where(a < 0, a + n, a)  # i == n: numpy's index -1 is the bottom level
        b = np.where(i == n, 0, a + 1)
        b = np.minimum(b, n - 1)  # (i == 0 takes `below`; keep the look-up in range)
        pick = lambda x, k: np.take_along_axis(x, k[np.newaxis, ...], axis=0)[0]
        pa, pb, da, db = pick(p_full, a), pick(p_full, b), pick(dphi, a), pick(dphi, b)
        above = pb + (tdphi - db) / (da - db) * (pa - pb)
    return np.where(i == 0, below, above)


def dewpoint_from_specific_humidity(q, p):
    """R: q_height.py:466-475: q == 0 -> EPS_SPECIFIC, e = p q / (eps + (1 - eps) q) (the oracle's form of the constant), then the
    inverse of the saturation formula over water (the oracle's dewpoint_from_relative_humidity)."""
    q = np.array(q, dtype=np.result_type(q, np.float32), copy=True)
    q[q == 0] = EPS_SPECIFIC
    eps = oracle.MET_EPSILON
    with np.errstate(all="ignore"):
        e = (p * q) / (eps + (eps * (1.0 / eps - 1.0)) * q)
        lnes = np.log(e / oracle.MET_C1)
        return (32.19 * lnes - 17.502 * oracle.MET_T0) / (lnes - 17.502)


def specific_humidity_from_dewpoint(td, p):
    """R: q_height.py:511-514: e = es_water(td), q = eps e / (p - (1 - eps) e), NaN where p - e < 1e-4."""
    eps = oracle.MET_EPSILON
    with np.errstate(all="ignore"):
        e = oracle.es_water(td)
        v = np.asarray(p - (1.0 - eps) * e).copy()
        v[np.asarray(p - e) < 1.0e-4] = np.nan
        return eps * e / v
