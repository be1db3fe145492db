"""The exact evaluator of tests/exact_statements.py on the CPU: its statements against the reference's own literals, its rounded
arguments against numpy's intermediates, its ulp measure, and the worst error of numpy's own arithmetic (oracle/oracle.py) on the
shared generators — what the GPU bounds of tests/test_gpu_ulp_budgets.py build on."""

from __future__ import annotations

import json
import math
import os

import mpmath
import numpy as np
import pytest

import exact_statements as X
from oracle import oracle

GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_vectors.json")))


def arr(v):
    return np.asarray(v, dtype=np.float64)


def f(values) -> np.ndarray:
    return np.array([float(v) for v in values])


def test_ulp_measure():
    f64, f32 = np.float64, np.float32
    one = mpmath.mpf(1)
    assert X.ulp_errors(np.array([1.0]), np.array([one], dtype=object), f64)[0] == 0
    assert X.ulp_errors(np.array([np.nextafter(1.0, 2.0)]), np.array([one], dtype=object), f64)[0] == 1
    # below a power of two the ulp is half as large: the ulp is that of the exact value ROUNDED
    assert X.ulp_errors(np.array([np.nextafter(1.0, 0.0)]), np.array([one], dtype=object), f64)[0] == 0.5
    assert X.ulp_errors(np.array([1.0], f32), np.array([one + mpmath.ldexp(1, -24)], dtype=object), f32)[0] == 0.5
    # subnormal results count in subnormal steps
    sub = 3 * 2.0**-1074
    assert X.ulp_errors(np.array([sub]), np.array([mpmath.mpf(5 * 2.0**-1074)], dtype=object), f64)[0] == 2
    assert X.ulp_errors(np.array([2.0**-149], f32), np.array([mpmath.ldexp(1, -150)], dtype=object), f32)[0] == 0.5
    assert X.round_to(mpmath.ldexp(3, -1076), f64) == 2.0**-1074  # 0.75 of the smallest step: up to it
    # overflow: a finite exact value beyond the dtype's range must come out as inf
    big = mpmath.exp(710)
    assert X.ulp_errors(np.array([np.inf, 1.7976931348623157e308]), np.array([big, big], dtype=object), f64).tolist() == [0, math.inf]
    assert X.round_to(mpmath.mpf(float(np.finfo(f32).max)) * (1 + mpmath.ldexp(1, -26)), f32) == float(np.finfo(f32).max)
    # special references match bit for bit: NaN, +-inf, the sign of zero
    got = np.array([np.nan, np.inf, -0.0, 0.0, 1.0])
    want = np.array([math.nan, math.inf, -0.0, -0.0, math.nan], dtype=object)
    assert X.ulp_errors(got, want, f64).tolist() == [0, 0, 0, math.inf, math.inf]


def test_arguments_round_like_numpy():
    """The single-function references take the argument as the statement rounds it: the restated roundings equal numpy's bits."""
    rng = np.random.default_rng(0)
    for dt in (np.float32, np.float64):
        x = rng.uniform(-1000.0, 1000.0, 20000).astype(dt)
        assert np.array_equal(X.argument_deg2rad(x), np.deg2rad(x))
        assert np.array_equal(x * dt(X.rad2deg_factor(dt)), np.rad2deg(x))
        d = rng.uniform(0.0, 360.0, 20000).astype(dt)
        assert np.array_equal(X.argument_polar(d), ((270.0 - d) * (np.pi / 180.0)).astype(dt))
        sd, rsn = rng.uniform(0.0, 0.3, 20000).astype(dt), rng.uniform(50.0, 600.0, 20000).astype(dt)
        before = np.clip(np.tanh(X.argument_snow_cover(sd, rsn)), 0, 1)  # the statement up to its jump, on the restated argument
        below = before <= 0.99
        assert before.dtype == dt and below.sum() > 1000 and np.array_equal(before[below], oracle.snow_cover(sd, rsn)[below])
    # np.rad2deg's float32 factor is 180f / pi_f, one ulp from float32(180 / pi): the exact direction_from_cos_sin uses numpy's
    assert X.rad2deg_factor(np.float32) == float(np.float32(180.0) / np.float32(np.pi))


def test_exact_statements_reproduce_the_reference_literals():
    """The exact humidity and uv <-> ddff statements at the reference's literals, at its tests' np.allclose.  (snow_cover has no literal
    in the reference's tests; its exact tanh is held against numpy's below.)"""
    k = X.consts(np.float64)
    d = GOLDEN["dewpoint"]
    r, t, td = arr(d["r"]).ravel(), arr(d["t"]).ravel(), arr(d["d"]).ravel()
    assert np.allclose(f(X.r_to_d_exact(k, *a) for a in zip(r, t)), td)
    assert np.allclose(f(X.d_to_r_exact(k, *a) for a in zip(td, t)), r)
    h = GOLDEN["pressure_level_humidity"]
    for level in h["levels"]:
        t, q, r = (arr(h[key][str(level)]).ravel() for key in ("t", "q", "r"))
        assert np.allclose(f(X.q_to_r_exact(k, qi, ti, 100.0 * level) for qi, ti in zip(q, t)), r)
        assert np.allclose(f(X.r_to_q_exact(k, ri, ti, 100.0 * level) for ri, ti in zip(r, t)), q)
    g = GOLDEN["uv_to_ddff"]
    for level in g["levels"]:
        u, v, ws, wdir = (arr(g[key][str(level)]).ravel() for key in ("u", "v", "ws", "wdir"))
        assert np.allclose(f(X.hypot_exact(a, b) for a, b in zip(u, v)), ws)
        assert np.allclose(f(X.polar_direction_exact(k, a, b) for a, b in zip(u, v)), wdir)
        a = X.argument_polar(wdir)
        assert np.allclose(f(X.polar_u_exact(s, x) for s, x in zip(ws, a)), u)
        assert np.allclose(f(X.polar_v_exact(s, x) for s, x in zip(ws, a)), v)


# numpy's own worst error (ulps; the direction of xy_to_polar in ulps of 360) on the shared generators, measured with the evaluator.
# Pinned within [0.8 x, 1.1 x + 0.1]: the composed GPU bounds are numpy's worst + a slack, so a generator that stopped reaching the
# ill-conditioned inputs — or a reference that started to — shows here first.
NUMPY_WORST = {
    ("exp", "float64", 0): 0.65, ("log", "float64", 0): 0.52, ("cos_sin", "float64", 0): 0.56, ("cos_sin", "float64", 1): 0.51,
    ("cos_sin_deg", "float64", 0): 0.56, ("cos_sin_deg", "float64", 1): 0.50, ("atan2", "float64", 0): 0.63,
    ("snow_cover", "float64", 0): 1.15, ("polar_to_xy", "float64", 0): 1.23, ("polar_to_xy", "float64", 1): 1.25,
    ("atan2_deg", "float64", 0): 1.23, ("xy_to_polar", "float64", 0): 0.59, ("xy_to_polar", "float64", 1): 1.00,
    ("r_to_d", "float64", 0): 2.04, ("d_to_r", "float64", 0): 53.57, ("q_to_r", "float64", 0): 33.99, ("r_to_q", "float64", 0): 33.06,
    ("q_to_r_level", "float64", 0): 31.18, ("r_to_q_level", "float64", 0): 33.61,
    ("exp", "float32", 0): 2.00, ("log", "float32", 0): 2.42, ("cos_sin", "float32", 0): 1.19, ("cos_sin", "float32", 1): 1.28,
    ("cos_sin_deg", "float32", 0): 1.08, ("cos_sin_deg", "float32", 1): 1.23, ("atan2", "float32", 0): 2.60,
    ("snow_cover", "float32", 0): 1.30, ("polar_to_xy", "float32", 0): 1.60, ("polar_to_xy", "float32", 1): 1.74,
    ("atan2_deg", "float32", 0): 2.52, ("xy_to_polar", "float32", 0): 0.50, ("xy_to_polar", "float32", 1): 1.18,
    ("r_to_d", "float32", 0): 2.63, ("d_to_r", "float32", 0): 79.16, ("q_to_r", "float32", 0): 28.70, ("r_to_q", "float32", 0): 31.42,
    ("q_to_r_level", "float32", 0): 31.72, ("r_to_q_level", "float32", 0): 34.66,
}


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", X.ALL)
def test_numpy_worst_error_is_pinned(name, dtype):
    st = X.statement(name, dtype)
    for out in range(len(st.exact)):
        err = st.numpy_errors(out)
        assert np.isfinite(err).all(), f"{name} output {out}: numpy's special values differ from the exact statement's"
        pinned = NUMPY_WORST[(name, np.dtype(dtype).name, out)]
        worst = float(err.max())
        print(f"{name} {np.dtype(dtype).name} out{out}: numpy {worst:.3f} ulps")
        assert 0.8 * pinned <= worst <= 1.1 * pinned + 0.1, (name, out, worst, pinned)


def test_generators_reach_their_edges():
    """The shared cases hold what they are for: both sides of the r_to_q guard band, the snow-cover jump, exact wraps, the phase ends."""
    for dt in (np.float64, np.float32):
        st = X.statement("r_to_q", dt)
        band = st.alt[0][0]
        assert band.sum() >= 16 and np.isnan(st.numpy_out[0].reshape(-1)[band]).any() and np.isfinite(st.numpy_out[0].reshape(-1)[band]).any()
        sc = X.statement("snow_cover", dt)
        assert sc.alt[0][0].any() or (sc.numpy_out[0] == 1.0).any()
        t = X.statement("q_to_r", dt).inputs[1].reshape(-1)
        for end in (X.MET_TI, X.MET_T0):
            assert (t == dt(end)).any() and (t < dt(end)).any() and (t > dt(end)).any()
        d = X.statement("atan2_deg", dt).numpy_out[0]
        assert ((d > 359.9) & (d < 360)).any() and ((d >= 0) & (d < 0.1)).any()
