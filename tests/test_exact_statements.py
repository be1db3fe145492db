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
import vertical_restatement as vr
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
    ("q_to_r_level", "float64", 0): 31.18, ("r_to_q_level", "float64", 0): 33.61, ("q_to_d", "float64", 0): 1.89, ("d_to_q", "float64", 0): 23.69,
    ("exp", "float32", 0): 2.00, ("log", "float32", 0): 2.42, ("cos_sin", "float32", 0): 1.19, ("cos_sin", "float32", 1): 1.28,
    ("cos_sin_deg", "float32", 0): 1.08, ("cos_sin_deg", "float32", 1): 1.23, ("atan2", "float32", 0): 2.60,
    ("snow_cover", "float32", 0): 1.30, ("polar_to_xy", "float32", 0): 1.60, ("polar_to_xy", "float32", 1): 1.74,
    ("atan2_deg", "float32", 0): 2.52, ("xy_to_polar", "float32", 0): 0.50, ("xy_to_polar", "float32", 1): 1.18,
    ("r_to_d", "float32", 0): 2.63, ("d_to_r", "float32", 0): 79.16, ("q_to_r", "float32", 0): 28.70, ("r_to_q", "float32", 0): 31.42,
    ("q_to_r_level", "float32", 0): 31.72, ("r_to_q_level", "float32", 0): 34.66, ("q_to_d", "float32", 0): 1.99, ("d_to_q", "float32", 0): 39.15,
}

# The column statement (pressure_at_height_levels): numpy's worst per (n_lev, group of cases, height class) as (float64, float32) — the
# restatement's float64 value against the exact one, rounded once to float32 for the second figure.  From numpy, never from the kernel.
NUMPY_WORST_COLUMN = {
    (1, "physical", "near ground"): (0.50, 0.5000), (1, "physical", "100 m"): (0.50, 0.4993), (1, "physical", "aloft"): (1.76, 0.5000), (1, "physical", "above top"): (0.00, 0.0000),
    (1, "bent and special", "near ground"): (0.50, 0.4981), (1, "bent and special", "100 m"): (0.52, 0.4988), (1, "bent and special", "aloft"): (1.19, 0.4992), (1, "bent and special", "above top"): (0.00, 0.0000),
    (2, "physical", "near ground"): (244.22, 0.4998), (2, "physical", "100 m"): (1.90, 0.4988), (2, "physical", "aloft"): (1.86, 0.4999), (2, "physical", "above top"): (3.11, 0.4994),
    (2, "bent and special", "near ground"): (206.51, 0.4986), (2, "bent and special", "100 m"): (52.56, 0.4976), (2, "bent and special", "aloft"): (76.41, 0.4997), (2, "bent and special", "above top"): (111.16, 0.4909),
    (3, "physical", "near ground"): (0.50, 0.4990), (3, "physical", "100 m"): (0.51, 0.4967), (3, "physical", "aloft"): (78.06, 0.4988), (3, "physical", "above top"): (9.03, 0.4984),
    (3, "bent and special", "near ground"): (55.34, 0.4997), (3, "bent and special", "100 m"): (43.42, 0.4914), (3, "bent and special", "aloft"): (40.06, 0.4987), (3, "bent and special", "above top"): (11.08, 0.4991),
    (60, "physical", "near ground"): (0.92, 0.4998), (60, "physical", "100 m"): (8.17, 0.4992), (60, "physical", "aloft"): (95.31, 0.4999), (60, "physical", "above top"): (37.12, 0.4945),
    (60, "bent and special", "near ground"): (173.85, 0.4971), (60, "bent and special", "100 m"): (145.41, 0.4999), (60, "bent and special", "aloft"): (148.88, 0.4997), (60, "bent and special", "above top"): (50.59, 0.4932),
    (137, "physical", "near ground"): (3.81, 0.4997), (137, "physical", "100 m"): (65.99, 0.4913), (137, "physical", "aloft"): (483.67, 0.4971), (137, "physical", "above top"): (95.63, 0.4994),
    (137, "bent and special", "near ground"): (202.68, 0.4988), (137, "bent and special", "100 m"): (220.54, 0.4980), (137, "bent and special", "aloft"): (395.59, 0.4996), (137, "bent and special", "above top"): (78.40, 0.4926),
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
        st = X.statement("d_to_q", dt)
        band, out = st.alt[0][0], st.numpy_out[0].reshape(-1)
        assert band.sum() >= 16 and np.isnan(out[band]).any() and np.isfinite(out[band]).any()
        assert np.isnan(out[(st.case.reshape(-1) == "atmosphere") & ~band]).any()  # the guard's NaN away from the band, too
        q = X.statement("q_to_d", dt).inputs[0].reshape(-1)
        assert (q == 0).sum() >= 16 and ((q > 0) & (q < np.finfo(dt).tiny)).sum() >= 16


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n_lev", X.COLUMN_N_LEV)
def test_column_generators_reach_their_edges(n_lev, dtype):
    """Every case takes each branch of the statement over its heights; the bent case holds columns that walk a second time in the
    kernel (a is not the first level from the bottom that does not count) at two heights or more, some of them with the negative
    temperature below or at the level found; the specials give NaN, and a finite value under a NaN that sits above the level found."""
    st = X.column_statement(dtype, n_lev)
    n = n_lev
    for name, (t, q, sp) in st.cases.items():
        with np.errstate(all="ignore"):
            dphi = X.numpy_dphi(t, q, sp, st.A, st.B)
        i = np.stack([(X.tdphi_of(h) > dphi).sum(axis=0) for h, _ in st.heights])
        assert (i == 0).any() and (i == n).any(), (name, n)
        assert n == 1 or ((i > 0) & (i < n)).any(), (name, n)
        if name in ("atmosphere", "standard profile"):
            assert (i[4] == 0).all()  # the negative height: below the ground
            assert not any(X.second_walk(dphi, X.tdphi_of(h)).any() for h, _ in st.heights) or name == "atmosphere"
        if name == "atmosphere":
            assert (q[:, :7] == 0).all()
        if name == "standard profile":
            assert (np.diff(dphi, axis=0) < 0).all()  # strictly monotone: growing upward
        if name == "bent" and n > 1:
            walks = [X.second_walk(dphi, X.tdphi_of(h)) for h, _ in st.heights]
            assert sum(w.sum() >= 4 for w in walks) >= 2, [int(w.sum()) for w in walks]
            under = 0  # second-walk columns whose negative temperature is at the level found (a) or below it
            for w, ij in zip(walks, i):
                for c in np.flatnonzero(w):
                    under += bool((t[n - 1 - ij[c]:, c] < 0).any())
            assert under >= 4
        if name == "specials":
            want = st.numpy_out[name]
            assert np.isnan(want).any() and np.isinf(sp).any() and (sp <= 0).any() and np.isnan(sp).any()
            assert (t[n - 1] == 0).any() and np.isnan(want[0][t[n - 1] == 0]).all()  # 0 / 0 at height 0
            bad = ~(np.isfinite(t) & np.isfinite(q))
            assert bad[0].any() and bad[n - 1].any() and bad[n // 2].any()
            if n > 1:  # a NaN at the top level, a finite result between two levels below it: the count was right
                nan_top = np.isnan(t[0]) | np.isnan(q[0])
                assert any((np.isfinite(w) & nan_top & (ij > 0) & (ij < n - 1)).any() for w, ij in zip(want, i)) or n == 2
                assert any((np.isfinite(w) & nan_top).any() for w in want)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n_lev", X.COLUMN_N_LEV)
def test_column_numpy_worst_error_is_pinned(n_lev, dtype):
    """The restatement against the exact column statement: its special values are the statement's, and its worst error per group of
    cases and height class is the pinned one — what the kernel's bounds (tests/test_gpu_column_ulps.py) are relative to."""
    st = X.column_statement(dtype, n_lev)
    for name in st.cases:
        for j in range(len(st.heights)):
            assert np.isfinite(st.numpy_errors(name, j)).all(), (name, st.heights[j], "numpy's special values differ from the exact statement's")
    for group in (X.PHYSICAL, X.ODD):
        for cls in X.HEIGHT_CLASSES:
            pinned = NUMPY_WORST_COLUMN[(n_lev, group, cls)][0 if dtype == np.float64 else 1]
            worst = st.numpy_worst(cls, group=group)
            print(f"column n_lev {n_lev} {group} {cls} {np.dtype(dtype).name}: numpy {worst:.4f} ulps")
            assert 0.8 * pinned <= worst <= 1.1 * pinned + 0.1, (n_lev, group, cls, worst, pinned)
            if dtype == np.float32:  # float64 throughout, one rounding: the restatement itself meets the kernel's float32 contract
                assert worst <= 0.5 + 1000 * 2.0**-29


def test_column_statement_constants_and_golden_path():
    """alpha[0] is the double numpy's log(2.0) gives (the kernel's kLn2 literal); the exact pressure at 2 m and the exact dewpoint of it
    reproduce the reference's Q2M -> D2M literals at its own rtol 1e-7."""
    assert X.LN2_F64 == 0.6931471805599453 == float.fromhex("0x1.62e42fefa39efp-1")
    g = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "height_level_humidity.json")))
    t = np.stack([np.array(g["t"][k]).ravel() for k in sorted(g["t"], key=int)])
    q = np.stack([np.array(g["q"][k]).ravel() for k in sorted(g["q"], key=int)])
    sp, q2m, d2m = (arr(g[k]).ravel() for k in ("sp", "q2m", "d2m"))
    A, B = X.hybrid_column(2)
    assert A.tolist() == g["AB"]["A"] and B.tolist() == g["AB"]["B"]
    exact, want = X.column_exact([2.0], t, q, sp, A, B)
    assert np.allclose(f(exact[0]), want[0], rtol=1e-12, atol=0)
    k = X.consts(np.float64)
    # (the exact dewpoint of the exact pressure rounded to float64: the pressure's rounding moves it by 1e-17 relative)
    td = f(X.q_to_d_exact(k, qi, float(pi)) for qi, pi in zip(q2m, exact[0]))
    np.testing.assert_allclose(td, d2m, rtol=1e-7, atol=0)
    # d_to_q undoes it (where q2m is not the zero that q_to_d replaced)
    back = f(X.d_to_q_exact(k, float(ti), float(pi)) for ti, pi in zip(td, exact[0]))
    np.testing.assert_allclose(back[q2m != 0], q2m[q2m != 0], rtol=1e-12)


@pytest.mark.parametrize("n_lev", [2, 3, 60, 137])
def test_column_statement_is_continuous_across_its_branches(n_lev):
    """One float64 step of tdphi either side of dphi[k] — k the bottom level (`below` meets `above`), an interior one (adjacent
    segments), the top (the wrap a = n-1, b = 0) — moves the exact value by no more than the steeper of the two segments' slopes times
    the step.  A shifted a or b, or a count off by one, jumps by a whole layer instead."""
    st = X.column_statement(np.float64, n_lev)
    t, q, sp = st.cases["standard profile"]
    dphi = X.numpy_dphi(t, q, sp, st.A, st.B)
    n = n_lev
    for c in range(0, 16):
        prof = X.ColumnProfile(t[:, c], q[:, c], float(sp[c]), st.A, st.B)
        pf, d = prof.p_full, prof.dphi
        slopes = [abs((prof.p_full[n - 1] - prof.p_half[n]) / d[n - 1])]  # `below`, then the segments (k, k + 1), then the wrap
        slopes += [abs((pf[k] - pf[k + 1]) / (d[k] - d[k + 1])) for k in range(n - 2, -1, -1)]
        slopes += [abs((pf[n - 1] - pf[0]) / (d[n - 1] - d[0]))]
        for k in sorted({n - 1, n // 2, 0}):
            centre = float(d[k])
            lo, hi = np.nextafter(centre, -np.inf), np.nextafter(centre, np.inf)
            lo, hi = (float(np.nextafter(lo, -np.inf)), float(hi)) if lo >= d[k] else (float(lo), float(hi) if hi > d[k] else float(np.nextafter(hi, np.inf)))
            assert prof.count(hi, dphi[:, c]) == prof.count(lo, dphi[:, c]) + 1 == n - k
            below, above = prof.value(lo, dphi[:, c], math.nan), prof.value(hi, dphi[:, c], math.nan)
            j = n - 1 - k  # the boundary between slopes[j] (under dphi[k]) and slopes[j + 1] (over it)
            bound = max(slopes[j], slopes[j + 1]) * (mpmath.mpf(hi) - mpmath.mpf(lo))
            assert abs(above - below) <= bound + abs(pf[k]) * mpmath.mpf(2) ** -118, (  # (+ the evaluator's own 128-bit rounding)
                n, c, k, float(abs(above - below)), float(bound))
            assert abs(below - pf[k]) <= bound and abs(above - pf[k]) <= bound  # and both sit at the full level's pressure


def test_column_exact_handles_special_levels():
    """What the evaluator does where the statement has no finite value, on a three-level column."""
    A, B = X.hybrid_column(3)
    t, q, sp = np.full((3, 1), 250.0), np.full((3, 1), 1e-3), np.array([1.0e5])
    dphi = X.numpy_dphi(t, q, sp, A, B)[:, 0]
    hs = [0.0, 2.0, dphi[1] / vr.G * 1.01, dphi[0] / vr.G * 2.0]
    base, want = X.column_exact(hs, t, q, sp, A, B)
    assert np.allclose(f(base.ravel()), want.ravel(), rtol=1e-12, atol=0)
    for level, v in ((0, np.nan), (0, np.inf), (1, np.nan), (2, -np.inf), (2, np.nan)):
        tt = t.copy()
        tt[level, 0] = v
        with np.errstate(all="ignore"):
            exact, want = X.column_exact(hs, tt, q, sp, A, B)
        for x, w in zip(exact.ravel(), want.ravel()):
            if isinstance(x, float):
                assert (math.isnan(x) and math.isnan(w)) or x == w, (level, v, x, w)
            else:
                assert abs(float(x) - w) <= 1e-12 * abs(w), (level, v, x, w)
    with np.errstate(all="ignore"):
        one, want = X.column_exact([0.0, 2.0, 1e6], np.full((1, 1), 250.0), np.zeros((1, 1)), sp, *X.hybrid_column(1))
    assert math.isnan(one[2, 0]) and np.isnan(want[2, 0]) and float(one[0, 0]) == 1.0e5  # n_lev == 1 above the level: da == db
