"""q_to_r_height / r_to_q_height / q_to_d_height / d_to_q_height (filters/domain.py) and the column kernel under them,
``atx_pressure_at_height_stack`` (csrc/atx_vertical.hip), against the restatement of tests/vertical_restatement.py.

The filter tests mirror the reference's (R: tests/field_filters/test_height_level_humidity.py), on its literals
(tests/golden/height_level_humidity.json), once through a CPU stand-in of the two native entry points they use and once on the GPU.
What the literals pin and what they cannot: the Q2M -> D2M dewpoints at the reference's own rtol 1e-7; the D2M -> Q2M humidities
at 5e-7 only; the R2M / Q2M literals not at all (the saturation-pressure restatement shared with q_to_r misses them by up to 4 %,
whatever the pressure — the filter says so at construction), so those cases are held to the restatement instead."""

from __future__ import annotations

import json
import logging
import os

import numpy as np
import pytest
import torch

from anemoi_transform_amd import native
from anemoi_transform_amd.filters import create_filter_by_name, filter_registry
from anemoi_transform_amd.filters import domain
from oracle import oracle

import native_double
import vertical_restatement as vr
from exact_statements import hybrid_column, second_walk
from test_domain_filters import fields_equal, select, test_source_from
from test_filters import collect_fields_by_param, test_source

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "height_level_humidity.json")))
MD = {"latitudes": GOLDEN["latitudes"], "longitudes": GOLDEN["longitudes"], "valid_datetime": GOLDEN["valid_datetime"]}
AB = GOLDEN["AB"]
NAMES = ("q_to_r_height", "r_to_q_height", "q_to_d_height", "d_to_q_height")


def arr(key):
    return np.array(GOLDEN[key], dtype=np.float64)


T_ML = {int(k): np.array(v) for k, v in GOLDEN["t"].items()}
Q_ML = {int(k): np.array(v) for k, v in GOLDEN["q"].items()}


# ---- CPU stand-in of the two entry points the filters call ----------------------------------------------------------------------
def pressure_at_height_stack(t, q, sp, A, B, out, *, n_pts, n_lev, pitch, layout, height):
    tt = native_double._levels(t, n_pts, n_lev, layout)
    qq = native_double._levels(q, n_pts, n_lev, layout)
    p = vr.pressure_at_height_levels(height, tt, qq, sp.numpy()[:n_pts], A.numpy(), B.numpy())
    out.numpy()[:n_pts] = p.astype(out.numpy().dtype)


def combine_stack(op, inputs, outputs, **kw):
    if op not in (native.COMB_Q_TO_D, native.COMB_D_TO_Q):
        return native_double.combine_stack(op, inputs, outputs, **kw)
    xs = [native_double._levels(x, kw["n_pts"], kw["n_lev"], kw["layout"]) for x in inputs]
    ys = native_double._levels(outputs[0], kw["n_pts"], kw["n_lev"], kw["layout"])
    fn = vr.dewpoint_from_specific_humidity if op == native.COMB_Q_TO_D else vr.specific_humidity_from_dewpoint
    ys[:] = fn(xs[0], xs[1]).astype(ys.dtype)


@pytest.fixture(params=["double", pytest.param("hip", marks=pytest.mark.gpu)])
def engine(request, monkeypatch):
    if request.param == "double":
        native_double.install(monkeypatch)
        monkeypatch.setattr(native, "pressure_at_height_stack", pressure_at_height_stack)
        monkeypatch.setattr(native, "combine_stack", combine_stack)
    return request.param


def model_levels(levtype="ml"):
    specs = [{"param": "t", "levtype": levtype, "levelist": level, "values": v.copy(), **MD} for level, v in T_ML.items()]
    return specs + [{"param": "q", "levtype": levtype, "levelist": level, "values": v.copy(), **MD} for level, v in Q_ML.items()]


def source(*params, levtype="ml"):
    keys = {"2sh": "q2m", "2r": "r2m", "2d": "d2m", "2t": "t2m", "sp": "sp"}
    return test_source([{"param": p, "values": arr(keys[p]), **MD} for p in params] + model_levels(levtype))


def select_and_add(first, second, params, additional_params):
    """R: tests/utils `SelectAndAddFieldSource`: the fields of `params` from the first source, those of `additional_params` from the second."""
    return test_source_from([f for f in first if f.metadata("param") in params] +
                            [f for f in second if f.metadata("param") in additional_params])


def make(name, **kw):
    return create_filter_by_name(name, height=2, specific_humidity_at_height_level="2sh", surface_pressure="sp",
                                 specific_humidity_at_model_levels="q", temperature_at_model_levels="t", model_level_AB=AB, **kw)


RH = dict(relative_humidity_at_height_level="2r", temperature_at_height_level="2t")
DP = dict(dewpoint_temperature_at_height_level="2d")


def pressure_2m():
    """The restated pressure at 2 m at the literal points (levels ascending: 136 on top of 137)."""
    return vr.pressure_at_height_levels(2.0, np.stack([T_ML[136], T_ML[137]]), np.stack([Q_ML[136], Q_ML[137]]), arr("sp"), AB["A"], AB["B"])


def test_the_four_names_are_registered():
    for name in NAMES:
        assert name in filter_registry.registered, name


# ---- the reference's cases, on its literals --------------------------------------------------------------------------------------
def test_specific_humidity_to_dewpoint_temperature(engine):
    """R: test_height_level_humidity.py:424-451 — the Q2M -> D2M literals at the reference's own tolerance (rtol 1e-7, atol 0)."""
    src = source("2sh", "sp", "2t")
    inputs, out = collect_fields_by_param(src), collect_fields_by_param(src | make("q_to_d_height", **DP))
    assert set(inputs) == {"2sh", "2t", "sp", "t", "q"}
    assert set(out) == {"2sh", "2t", "sp", "2d"}
    for p in ("2sh", "2t", "sp"):
        assert all(fields_equal(a, b) for a, b in zip(inputs[p], out[p]))
    np.testing.assert_allclose(out["2d"][0].to_numpy(), arr("d2m"), rtol=1e-7, atol=0)
    # the EPS_SPECIFIC guard acts on the operand, not on the field passed on: the zero humidity comes back as zero
    assert out["2sh"][0].to_numpy()[0, 0] == 0.0 and np.array_equal(out["2sh"][0].to_numpy(), arr("q2m"))


def test_dewpoint_temperature_to_specific_humidity(engine):
    """R: test_height_level_humidity.py:574-596.  The D2M -> Q2M literals at 5e-7, not the reference's 1e-7: the best any pressure
    candidate reaches from the 8-digit dewpoints is 2.8e-7.  Where the literal is 0 the forward filter's EPS_SPECIFIC guard made the
    dewpoint of q = 1e-8, which cannot be undone: the result is 1e-8 there (atol 1e-10)."""
    src = source("2d", "sp")
    inputs, out = collect_fields_by_param(src), collect_fields_by_param(src | make("d_to_q_height", **DP))
    assert set(inputs) == {"2d", "sp", "t", "q"}
    assert set(out) == {"2d", "sp", "2sh"}
    for p in ("2d", "sp"):
        assert all(fields_equal(a, b) for a, b in zip(inputs[p], out[p]))
    got, want = out["2sh"][0].to_numpy(), arr("q2m")
    zero = want == 0
    np.testing.assert_allclose(got[~zero], want[~zero], rtol=5e-7, atol=0)
    np.testing.assert_allclose(got[zero], vr.EPS_SPECIFIC, rtol=0, atol=1e-10)


def test_specific_humidity_to_relative_humidity(engine):
    """R: test_height_level_humidity.py:163-192, with the restatement in place of the R2M literals (see the module docstring)."""
    src = source("2sh", "sp", "2t")
    inputs, out = collect_fields_by_param(src), collect_fields_by_param(src | make("q_to_r_height", **RH))
    assert set(inputs) == {"2sh", "2t", "sp", "t", "q"}
    assert set(out) == {"2sh", "2t", "sp", "2r"}
    for p in ("2sh", "2t", "sp"):
        assert all(fields_equal(a, b) for a, b in zip(inputs[p], out[p]))
    want = oracle.relative_humidity_from_specific_humidity(arr("t2m"), arr("q2m"), pressure_2m())
    np.testing.assert_allclose(out["2r"][0].to_numpy(), want, rtol=1e-13)


def test_relative_humidity_to_specific_humidity(engine):
    """R: test_height_level_humidity.py:294-321, with the restatement in place of the Q2M literals."""
    src = source("2r", "sp", "2t")
    inputs, out = collect_fields_by_param(src), collect_fields_by_param(src | make("r_to_q_height", **RH))
    assert set(inputs) == {"2r", "2t", "sp", "t", "q"}
    assert set(out) == {"2r", "2t", "sp", "2sh"}
    for p in ("2r", "2t", "sp"):
        assert all(fields_equal(a, b) for a, b in zip(inputs[p], out[p]))
    want = oracle.specific_humidity_from_relative_humidity(arr("t2m"), arr("r2m"), pressure_2m())
    np.testing.assert_allclose(out["2sh"][0].to_numpy(), want, rtol=1e-13)


@pytest.mark.parametrize("first,second,params,kw,start,middle,out_params", [
    ("q_to_r_height", "r_to_q_height", ["2r", "2t", "sp"], RH, ("2sh", "sp", "2t"), {"2r", "2t", "sp", "t", "q"}, {"2sh", "2r", "2t", "sp"}),
    ("r_to_q_height", "q_to_r_height", ["2sh", "2t", "sp"], RH, ("2r", "sp", "2t"), {"2sh", "2t", "sp", "t", "q"}, {"2sh", "2r", "2t", "sp"}),
    ("q_to_d_height", "d_to_q_height", ["2d", "sp"], DP, ("2sh", "sp", "2t"), {"2d", "2t", "sp", "t", "q"}, {"2sh", "2t", "2d", "sp"}),
    ("d_to_q_height", "q_to_d_height", ["2sh", "sp"], DP, ("2d", "sp"), {"2sh", "sp", "t", "q"}, {"2sh", "2d", "sp"}),
], ids=["q-r-q", "r-q-r", "q-d-q", "d-q-d"])
def test_round_trips(engine, first, second, params, kw, start, middle, out_params):
    """R: test_height_level_humidity.py:195-250, :324-379, :454-510, :599-654 — the fields of the start come back from the round trip
    (`assert_fields_equal`: np.allclose), and the intermediate fields pass the second filter unchanged."""
    src = source(*start)
    extra = ["2t", "q", "t"] if first == "q_to_d_height" else ["q", "t"]
    mid = select_and_add(list(src | make(first, **kw)), list(src), params, extra)
    inputs, intermediate = collect_fields_by_param(src), collect_fields_by_param(mid)
    out = collect_fields_by_param(mid | make(second, **kw))
    assert set(intermediate) == middle and set(out) == out_params
    for p in set(start):
        assert all(fields_equal(a, b) for a, b in zip(inputs[p], out[p])), p
    for p in params:
        assert all(fields_equal(a, b) for a, b in zip(intermediate[p], out[p])), p


# ---- construction and consistency errors (R: q_height.py:28-54) ---------------------------------------------------------------------
def test_model_level_AB_names_and_types():
    for name in ("IFS_137", "ifs_137", "L91"):
        with pytest.raises(KeyError, match="is not in the list of predefined AB-coefficients") as info:
            create_filter_by_name("q_to_d_height", model_level_AB=name)
        assert "not bundled" in str(info.value) and "register_model_level_AB" in str(info.value)
    for bad in ([AB["A"], AB["B"]], (1, 2), 137):
        with pytest.raises(TypeError, match="model_level_AB must be a string or a dictionary."):
            create_filter_by_name("q_to_r_height", model_level_AB=bad)
    domain.register_model_level_AB("test_l2", AB["A"], AB["B"])
    try:
        f = create_filter_by_name("q_to_d_height", model_level_AB="TEST_L2", specific_humidity_at_height_level="2sh")
        assert list(f.A) == AB["A"] and list(f.B) == AB["B"]
    finally:
        domain.MODEL_LEVEL_AB.pop("TEST_L2")


def test_consistency_assertions(engine):
    with pytest.raises(AssertionError, match="does not contain model levels"):
        list(source("2sh", "sp", levtype="pl") | make("q_to_d_height", **DP))
    for A, B in ((AB["A"][1:], AB["B"][1:]), (AB["A"] + [0.0], AB["B"] + [1.0])):
        with pytest.raises(AssertionError, match="one more vertical level"):
            list(source("2sh", "sp") | create_filter_by_name("q_to_d_height", specific_humidity_at_height_level="2sh", dewpoint_temperature_at_height_level="2d",
                                                            model_level_AB={"A": A, "B": B}))
    with pytest.raises(AssertionError, match="same shape"):
        list(source("2sh", "sp") | create_filter_by_name("q_to_d_height", specific_humidity_at_height_level="2sh", model_level_AB={"A": AB["A"], "B": AB["B"][1:]}))


def test_parity_notes(caplog):
    from anemoi_transform_amd.core import reset_notes

    for name, gap in (("q_to_r_height", True), ("r_to_q_height", True), ("q_to_d_height", False), ("d_to_q_height", False)):
        reset_notes()
        caplog.clear()
        with caplog.at_level(logging.DEBUG, logger="anemoi_transform_amd"):
            create_filter_by_name(name, model_level_AB=AB)
        notes = [r.getMessage() for r in caplog.records if r.levelno >= logging.WARNING and "pinned" in r.getMessage()]
        assert len(notes) == 1 and "earthkit-meteo" in notes[0] and "reference's test points" in notes[0] and "np.allclose" in notes[0]
        assert ("4.3 %" in notes[0]) == gap


# ---- the restatement against an independent route --------------------------------------------------------------------------------
def sigma_column(n):
    """Half levels of a terrain-following column: B from 0 (top) to 1 (ground), geometric towards the top, A = 0."""
    B = np.concatenate([[0.0], np.geomspace(1e-3, 1.0, n)])
    return np.zeros(n + 1), B


def test_restatement_on_an_isothermal_dry_hydrostatic_column():
    """An isothermal (280 K), dry (q = 0) column of 137 levels: the hydrostatic pressure at height z is sp exp(-u), u = g z / (Rd T).

    Below the lowest full level (here ~206 m: z = 2, 10, 100 m) the statement interpolates p linearly in the geopotential between the
    surface (0, sp) and the lowest full level (u_f Rd T, p_full), u_f = alpha[n-1] — the IFS discretisation's own full-level
    geopotential.  For the convex exp(-u) the chord lies above the curve by at most u (u_f - u) / 2 (relative to sp), and the end point
    is off the curve by m = p_full / sp - exp(-u_f), which the chord carries in proportion u / u_f: the bound asserted is
    u (u_f - u) / 2 + (u / u_f) |m| + 1e-14, divided by exp(-u).

    Above it (z = 1000 m) the statement accumulates alpha (~ delta / 2) where the hydrostatic integral accumulates delta = ln of the
    half-level pressure ratio: its geopotentials come out about half the hydrostatic ones, and p lies between the hydrostatic column
    and the half-thickness column sp exp(-2 u), the latter within one layer (delta_max).  A flipped or shifted level index lands far
    outside both."""
    n, T = 137, 280.0
    A, B = sigma_column(n)
    sp = np.array([101325.0, 85000.0, 60000.0])
    t, q = np.full((n, sp.size), T), np.zeros((n, sp.size))
    ph = A[:, None] + B[:, None] * sp
    alpha_bottom = 1.0 - ph[n - 1] / (ph[n] - ph[n - 1]) * np.log(ph[n] / ph[n - 1])
    p_full_bottom = (ph[n - 1] + ph[n]) / 2.0
    u_f = alpha_bottom
    m = np.abs(p_full_bottom / sp - np.exp(-u_f))
    for z in (2.0, 10.0, 100.0):
        u = vr.G * z / (vr.RD * T)
        assert (u < u_f).all()  # below the lowest full level
        got = vr.pressure_at_height_levels(z, t, q, sp, A, B)
        bound = (u * (u_f - u) / 2.0 + (u / u_f) * m + 1e-14) / np.exp(-u)
        assert (np.abs(got / (sp * np.exp(-u)) - 1.0) <= bound).all(), (z, np.abs(got / (sp * np.exp(-u)) - 1.0), bound)
    z = 1000.0
    u = vr.G * z / (vr.RD * T)
    delta_max = np.log(ph[2:] / ph[1:-1]).max()
    got = vr.pressure_at_height_levels(z, t, q, sp, A, B)
    assert (got < sp * np.exp(-u)).all() and (got > sp * np.exp(-2.0 * u) * (1.0 - delta_max)).all()


def test_restatement_above_the_top_level_wraps_as_numpy_does():
    """i == n (the height above the top full level): a = -1 is numpy's bottom level, b = 0 — the interpolation between the top and
    the bottom full levels, extended beyond the top."""
    n = 3
    A, B = np.array([0.0, 2000.0, 1000.0, 0.0]), np.array([0.0, 0.5, 0.8, 1.0])
    sp = np.array([100000.0])
    t, q = np.full((n, 1), 250.0), np.full((n, 1), 0.001)
    p_full, p_half, alpha = vr.pressure_at_model_levels(A, B, sp)
    dphi = vr.relative_geopotential_thickness(alpha, t, q)
    z = 2.0 * dphi[0, 0] / vr.G
    got = vr.pressure_at_height_levels(z, t, q, sp, A, B)[0]
    tdphi = z * vr.G
    want = p_full[0, 0] + (tdphi - dphi[0, 0]) / (dphi[n - 1, 0] - dphi[0, 0]) * (p_full[n - 1, 0] - p_full[0, 0])
    assert got == want and got < p_full[0, 0]


# ---- the kernels against the restatement (GPU) -----------------------------------------------------------------------------------
def random_columns(rng, n, n_pts, np_dtype):
    t = rng.uniform(200.0, 310.0, (n, n_pts))
    q = 10.0 ** rng.uniform(-6.0, -1.7, (n, n_pts))
    q[:, :7] = 0.0
    sp = rng.uniform(50000.0, 106000.0, n_pts)
    cols = rng.choice(n_pts, 60, replace=False)
    for j, c in enumerate(cols):  # NaN columns: a NaN at one level (the top, the bottom, any), or no surface pressure
        level = (0, n - 1, int(rng.integers(n)))[j % 3]
        (t if j % 2 == 0 else q)[level, c] = np.nan
    sp[cols[:6]] = np.nan
    bent = rng.choice(n_pts, 40, replace=False)  # dphi not monotone: a negative temperature somewhere (the kernel's second walk)
    t[rng.integers(n, size=bent.size), bent] = -rng.uniform(100.0, 900.0, bent.size)
    return t.astype(np_dtype), q.astype(np_dtype), sp.astype(np_dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("n_lev", [2, 3, 60, 137])
@pytest.mark.parametrize("np_dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("layout", [native.COLUMNS, native.FIELDS], ids=["columns", "fields"])
def test_pressure_kernel_vs_restatement(dev, n_lev, np_dtype, layout):
    """The larger-n_pts coverage of the column kernel (tests/test_gpu_column_ulps.py holds it in ulps against exact arithmetic).
    float64: the restatement at rtol 2e-13.  float32: that bound carried through the one rounding the kernel's contract allows —
    |got - want64| <= 0.5 ulp32(want64) + 2e-13 |want64|."""
    from anemoi_transform_amd.stack import Stack

    rng = np.random.default_rng(100 + n_lev)
    n_pts = 20011 if n_lev > 60 else 30011
    t, q, sp = random_columns(rng, n_lev, n_pts, np_dtype)
    A, B = hybrid_column(n_lev)
    ts, qs = Stack.from_fields(t, dev=dev, layout=layout), Stack.from_fields(q, dev=dev, layout=layout)
    spd = torch.from_numpy(sp).to(dev)
    Ad, Bd = torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev)
    p_full, _, alpha = vr.pressure_at_model_levels(A, B, sp)
    dphi = vr.relative_geopotential_thickness(alpha, t, q)
    top = np.nanmedian(dphi[0]) / vr.G
    heights = [0.0, 2.0, 10.0, 0.3 * top, 0.7 * top, 1.5 * top + 1000.0]
    counts = np.zeros(3, dtype=np.int64)  # i == 0, 0 < i < n, i == n
    walks = 0  # planted columns that take the kernel's second walk (a is not the first level that does not count)
    for h in heights:
        i = (h * vr.G > dphi).sum(axis=0)
        walks += int(second_walk(dphi, h * vr.G).sum())
        counts += [(i == 0).sum(), ((i > 0) & (i < n_lev)).sum(), (i == n_lev).sum()]
        out = torch.full((n_pts,), 7.0, dtype=ts.dtype, device=dev)
        native.pressure_at_height_stack(ts.data, qs.data, spd, Ad, Bd, out, n_pts=n_pts, n_lev=n_lev, pitch=ts.pitch, layout=layout, height=h)
        got = out.cpu().numpy()
        want64 = vr.pressure_at_height_levels(h, t, q, sp, A, B)
        with np.errstate(all="ignore"):
            want = want64.astype(np_dtype)
        assert got.dtype == np_dtype
        assert np.array_equal(np.isnan(got), np.isnan(want)), (h, np.flatnonzero(np.isnan(got) != np.isnan(want))[:10])
        ok = np.isfinite(want)
        if np_dtype == np.float64:
            np.testing.assert_allclose(got[ok], want[ok], rtol=2e-13, atol=0, err_msg=f"height {h}")
        else:
            bound = 0.5 * np.spacing(np.abs(want[ok])).astype(np.float64) + 2e-13 * np.abs(want64[ok])
            miss = np.abs(got[ok].astype(np.float64) - want64[ok]) > bound
            assert not miss.any(), (h, int(miss.sum()), got[ok][miss][:3], want64[ok][miss][:3])
    assert (counts > 0).all(), counts  # every branch of the statement was taken
    assert walks > 0, "no planted column takes the second walk at any height"


@pytest.mark.gpu
@pytest.mark.parametrize("np_dtype,rtol", [(np.float64, 2e-13), (np.float32, 2e-5)], ids=["f64", "f32"])
@pytest.mark.parametrize("layout", [native.COLUMNS, native.FIELDS], ids=["columns", "fields"])
def test_dewpoint_operators_vs_restatement(dev, np_dtype, rtol, layout):
    """ATX_COMB_Q_TO_D / ATX_COMB_D_TO_Q at the bounds the other humidity operators meet (tests/test_domain_filters.py)."""
    from anemoi_transform_amd.stack import Stack

    rng = np.random.default_rng(7)
    n_lev, n_pts = 3, 30011
    q = (10.0 ** rng.uniform(-7, -1.5, (n_lev, n_pts))).astype(np_dtype)
    q[0, :5] = 0.0  # the EPS_SPECIFIC guard
    td = rng.uniform(180.0, 310.0, (n_lev, n_pts)).astype(np_dtype)
    p = rng.uniform(500.0, 106000.0, (n_lev, n_pts)).astype(np_dtype)  # low pressures: e reaches p for warm dewpoints, the guard's NaN

    def run(op, a, b):
        sa, sb = Stack.from_fields(a, dev=dev, layout=layout), Stack.from_fields(b, dev=dev, layout=layout)
        out = sa.new_like(zero=False)
        native.combine_stack(op, [sa.data, sb.data], [out.data], n_pts=n_pts, n_lev=n_lev, pitch=sa.pitch, layout=layout)
        return out.numpy()

    for got, want in ((run(native.COMB_Q_TO_D, q, p), vr.dewpoint_from_specific_humidity(q, p)),
                      (run(native.COMB_D_TO_Q, td, p), vr.specific_humidity_from_dewpoint(td, p))):
        want = want.astype(np_dtype)
        assert got.dtype == np_dtype and np.array_equal(np.isnan(got), np.isnan(want))
        ok = np.isfinite(want)
        np.testing.assert_allclose(got[ok], want[ok], rtol=rtol)
    assert np.isnan(vr.specific_humidity_from_dewpoint(td, p)).any()


@pytest.mark.gpu
def test_o1280_137_levels_through_the_plugin_api(dev, monkeypatch):
    """O1280 with 137 model levels (float32, device-resident) -> 2r and 2d through create_filter_by_name: one column walk and one
    combine launch per filter, checked against the restatement on 4096 points."""
    from anemoi_transform_amd.fields import ArrayField, FieldList, new_field_from_stack
    from anemoi_transform_amd.grids import lookup
    from anemoi_transform_amd.stack import Stack

    n_lev, grid = 137, lookup("o1280")
    n_pts = len(grid["latitudes"])
    assert n_pts == 6599680
    A, B = hybrid_column(n_lev)
    g = torch.Generator(device=dev).manual_seed(5)
    t = Stack.empty(n_pts, n_lev, torch.float32, dev)
    q = Stack.empty(n_pts, n_lev, torch.float32, dev)
    t.data[:, :n_lev] = 200.0 + 100.0 * torch.rand(n_pts, n_lev, device=dev, generator=g)
    q.data[:, :n_lev] = torch.pow(10.0, -6.0 + 4.0 * torch.rand(n_pts, n_lev, device=dev, generator=g))
    single = Stack.empty(n_pts, 3, torch.float32, dev)
    single.data[:, 0] = 60000.0 + 45000.0 * torch.rand(n_pts, device=dev, generator=g)  # sp
    single.data[:, 1] = t.data[:, n_lev - 1] + 1.0  # 2t
    single.data[:, 2] = q.data[:, n_lev - 1] * 0.9  # 2sh
    template = ArrayField(np.zeros(1), {"param": "?"}, np.zeros(1), np.zeros(1))
    ll = dict(latitudes=grid["latitudes"], longitudes=grid["longitudes"])
    fields = [new_field_from_stack(single, j, template=template, metadata={"param": name}, **ll) for j, name in enumerate(("sp", "2t", "2sh"))]
    for name, st in (("t", t), ("q", q)):
        fields += [new_field_from_stack(st, k, template=template, metadata={"param": name, "levtype": "ml", "levelist": k + 1}, **ll)
                   for k in range(n_lev)]
    calls = {"pressure_at_height_stack": 0, "combine_stack": 0}
    for name in calls:
        real = getattr(native, name)

        def wrapped(*a, _real=real, _name=name, **k):
            calls[_name] += 1
            return _real(*a, **k)

        monkeypatch.setattr(native, name, wrapped)
    AB137 = {"A": A.tolist(), "B": B.tolist()}
    r = collect_fields_by_param(create_filter_by_name("q_to_r_height", model_level_AB=AB137, specific_humidity_at_height_level="2sh").forward(FieldList(fields)))
    d = collect_fields_by_param(create_filter_by_name("q_to_d_height", model_level_AB=AB137, specific_humidity_at_height_level="2sh").forward(FieldList(fields)))
    assert calls == {"pressure_at_height_stack": 2, "combine_stack": 2}
    assert set(r) == {"2sh", "2r", "2t", "sp"} and set(d) == {"2sh", "2d", "sp", "2t"}
    rng = np.random.default_rng(0)
    pts = torch.from_numpy(np.sort(rng.choice(n_pts, 4096, replace=False))).to(dev)
    th = t.data[pts, :n_lev].double().cpu().numpy().T
    qh = q.data[pts, :n_lev].double().cpu().numpy().T
    sp, t2, q2 = (single.data[pts, j].double().cpu().numpy() for j in range(3))
    p = vr.pressure_at_height_levels(2.0, th, qh, sp, A, B)
    got_r = r["2r"][0].to_numpy(flatten=True)[pts.cpu().numpy()]
    got_d = d["2d"][0].to_numpy(flatten=True)[pts.cpu().numpy()]
    assert got_r.dtype == np.float32 and got_d.dtype == np.float32
    np.testing.assert_allclose(got_r, oracle.relative_humidity_from_specific_humidity(t2, q2, p), rtol=2e-5)
    np.testing.assert_allclose(got_d, vr.dewpoint_from_specific_humidity(q2, p), rtol=2e-5)
