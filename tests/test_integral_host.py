"""``atx_integral_columns`` without a GPU: the numpy loop of include/atx_integral.h (tests/integral_statement.py) against the same loop in
exact arithmetic, within the bound the header derives, and against two closed forms; the library's table row and the refusals of its C
ABI that come before anything touches HIP; the ``ValueError``s of the ``vertical_integral`` filter.

numpy's own worst distance from exact, measured here on the CPU and printed, in ulps of sum |w f| / divisor: float64 2767.6 where a
layer of 10 Pa is cut out of one of 137 hybrid layers (K = max P / min dP is about 10^4 there: 0.0023 of the derived bound), at most
15.7 over the other cases, never more than 0.022 of the bound; float32 0.5000, its one rounding."""

from __future__ import annotations

import ctypes
import math

import numpy as np
import pytest

import __graft_entry__ as graft
import integral_statement as st
from anemoi_transform_amd import native, native_integral
from anemoi_transform_amd.filters import create_filter_by_name
from hybrid_column_common import WIDTHS, fields


@pytest.mark.parametrize("mode", [st.HYBRID, st.PRESSURE])
@pytest.mark.parametrize("shape", st.SHAPES, ids=lambda s: "-".join(map(str, s)))
@pytest.mark.parametrize("T", WIDTHS)
def test_the_loop_is_within_the_headers_bound_of_exact_arithmetic(T, shape, mode):
    c = st.case(np.dtype(T).name, shape, mode)
    points = sorted(set(range(min(12, shape[0]))) | set(range(0, shape[0], 5)))  # the planted points and every fifth
    for kind in (st.SUM, st.MEAN):
        y = st.reference(np.dtype(T).name, shape, mode, kind)
        worst, of_bound = st.worst_ulps(y, c["x"], c["sp"], c["terms"], c["bounds"], kind, c["A"], c["B"], c["P"], points)
        print(f"integral {np.dtype(T).name} {shape} {mode} {kind}: numpy {worst:.4f} ulps from exact, {of_bound:.3g} of the derived bound")
        assert of_bound <= 1.0
        if shape[0] > 9:
            assert np.isnan(y[7]).all() and np.isnan(y[9, 0, 0]) and not np.isnan(y[9, 1, 0])  # a NaN sp; a NaN above the ground shows in its own terms
            if mode == st.PRESSURE:  # NaN under the ground does not show; a column wholly under the ground is empty
                assert np.isfinite(y[10:, :, 0]).all() and (np.isnan(y[3]).all() if kind == st.MEAN else (y[3] == 0).all())
            if shape[4] >= 4:  # a bound wholly under the ground
                assert (np.isnan(y[10:, :, 3]).all() if kind == st.MEAN else (y[10:, :, 3] == 0).all())
    assert native_integral.ulps_f64(137, 3.0) == st.ulps_f64(137, 3.0, st.SUM) == 16.0 * 3.0 + 8 + 18 + 2 and (native_integral.BLOCK, native_integral.G) == (st.BLOCK, st.G)


def test_the_loop_gives_two_closed_forms():
    g = np.float64(st.G)
    A, B = st.table(12)
    sp = np.array([101325.0, 70000.0])
    for top, bottom in ((0.0, math.inf), (25000.0, 60000.0), (65000.0, 90000.0)):  # a constant column: x (c - a) / g
        y = st.statement(np.full((2, 1, 12), 3.5), sp, [(0, -1)], [(top, bottom)], st.SUM, A=A, B=B)[:, 0, 0]
        np.testing.assert_allclose(y, 3.5 * (np.minimum(bottom, sp) - top) / g, rtol=1e-13)
        assert (st.statement(np.full((2, 1, 12), 3.5), sp, [(0, -1)], [(top, bottom)], st.MEAN, A=A, B=B) == 3.5).all()
    P = np.array([10000.0, 25000.0, 50000.0, 70000.0, 85000.0, 100000.0])
    x = (2.0 + 3.0e-5 * P)[None, None, :].repeat(2, axis=0)
    x[1, 0, 4:] = np.nan  # sp = 70000 exactly on a level: the two levels under the ground are never read
    for top, bottom in ((10000.0, 70000.0), (30000.0, 60000.0), (26000.0, 27000.0)):  # linear in p on pl: the exact trapezoid
        y = st.statement(x, sp, [(0, -1)], [(top, bottom)], st.SUM, P=P)[:, 0, 0]
        np.testing.assert_allclose(y, (bottom - top) * (2.0 + 3.0e-5 * (top + bottom) / 2) / g, rtol=1e-13)
    y = st.statement(x, sp, [(0, -1), (0, 0)], [(0.0, math.inf)], st.SUM, P=P)  # held constant from the lowest level down to the ground
    assert y[0, 0, 0] == pytest.approx(((100000.0 - 10000.0) * (2.0 + 3.0e-5 * 55000.0) + 1325.0 * 5.0) / g, rel=1e-13)
    assert y[1, 0, 0] == pytest.approx((70000.0 - 10000.0) * (2.0 + 3.0e-5 * 40000.0) / g, rel=1e-13) and np.isfinite(y[1, 1, 0])


def test_the_library_row_and_the_refusals_that_need_no_gpu():
    """The refusals of include/atx_integral.h that are this library's own come before anything touches HIP: no pointer is dereferenced."""
    assert [lib.binding for lib in graft.LIBRARIES].count("native_integral") == 1
    lib = native_integral.load()
    assert lib.atx_integral_version() == 420 and (native_integral.MAX_LEVELS, native_integral.MAX_TERMS, native_integral.MAX_BOUNDS) == (256, 64, 32)
    at = lambda address: ctypes.c_void_p(address)  # noqa: E731
    ints, doubles = lambda *v: (ctypes.c_int32 * len(v))(*v), lambda *v: (ctypes.c_double * len(v))(*v)  # noqa: E731

    def call(out=at(3 << 20), terms=ints(0, -1, 1, 0), bounds=doubles(0.0, math.inf), A=at(80), P=None, n_pts=8, n_var=2, n_lev=4, n_term=2, src_pitch=8, dtype=0, mode=0):
        return lib.atx_integral_columns(at(1 << 20), at(2 << 20), out, terms, bounds, A, at(160), P, n_pts, n_var, n_lev, n_term, 1, src_pitch, 2, dtype, 0, mode, 0, None)

    said = lambda: lib.atx_integral_last_error().decode()  # noqa: E731
    assert call(n_pts=0) == native.OK and call(n_term=0, terms=None, out=None) == native.OK
    for terms in (ints(0, -1, 2, 0), ints(0, 2, 1, 0), ints(-1, 0, 1, 0)):
        assert call(terms=terms) == native.EINVAL and "is outside the 2 variables" in said()
    for bounds in (doubles(-1.0, 5.0), doubles(5.0, 5.0), doubles(math.nan, 5.0), doubles(0.0, math.nan)):
        assert call(bounds=bounds) == native.EINVAL and "is not 0 <= top < bottom" in said()
    assert call(n_lev=257, src_pitch=514) == native.ENOTIMPL and "exceeds the 256 levels of one call" in said()
    assert call(n_term=65, terms=ints(*[0, -1] * 65)) == native.ENOTIMPL and "exceed the 64 terms and 32 bounds" in said()
    assert call(A=None) == native.EINVAL and "null A / B table" in said() and call(mode=1) == native.EINVAL and "null levels_pa" in said()
    assert call(out=at((1 << 20) + 100)) == native.EINVAL and "out overlaps src" in said() and call(out=at((2 << 20) + 28)) == native.EINVAL and "out overlaps sp" in said()
    assert call(n_var=250, n_lev=256, src_pitch=64000, dtype=1, out=at(1 << 40)) == native.ENOTIMPL and "bytes of LDS, a workgroup has 65536" in said()


Q, U = [("q", "ml", k) for k in (3, 4, 5)], [("u", "ml", k) for k in (3, 4, 5)]
AB = dict(A=[0.0, 2000.0, 6000.0, 9000.0, 6000.0, 0.0], B=[0.0, 0.0, 0.1, 0.4, 0.8, 1.0])
SP = ("sp", "sfc", None)


def test_the_filter_checks_its_configuration_and_groups_before_any_launch():
    """Host fields, no GPU here: each of these raises from the bookkeeping, before a stack is built or a kernel launched."""
    make = lambda **k: create_filter_by_name("vertical_integral", **{**dict(outputs={"tcwv": "q", "viwve": ["q", "u"]}, model_level_AB=AB), **k})  # noqa: E731
    f = make(layers=[[850, 500], [300.5, 700]])
    assert (f.params, f.terms, f.bounds_pa) == (["q", "u"], [(0, -1), (0, 1)], [(50000.0, 85000.0), (30050.0, 70000.0)])
    assert f.output_names() == ["tcwv_850_500", "tcwv_300.5_700", "viwve_850_500", "viwve_300.5_700"] and make().output_names() == ["tcwv", "viwve"]
    for wrong, message in ((dict(levtype="hl"), "levtype must be 'ml' or 'pl'"), (dict(model_level_AB=None), "needs model_level_AB"),
                           (dict(levtype="pl"), "takes no table"), (dict(kind="median"), "kind must be one of 'integral', 'mean'"),
                           (dict(outputs={}), "non-empty dict"), (dict(outputs={"x": ["q", "u", "v"]}), "one param or two"),
                           (dict(layers=[[500, 500]]), "two different pressures"), (dict(outputs={"x": "sp"}), "not one of the params it weighs")):
        with pytest.raises(ValueError, match=f"vertical_integral: .*{message}"):
            make(**wrong)
    for specs, message in (((*Q, *U[1:], SP), r"mixed level sets for q and u: \[3, 4, 5\] and \[4, 5\]"),
                           ((*Q, SP), r"mixed level sets for q and u: \[3, 4, 5\] and \[\]"),
                           ((Q[0], Q[2], U[0], U[2], SP), r"not one run of the A / B table: missing levels \[4\]"),
                           ((*Q, *U), "no surface pressure 'sp'"), ((*Q, *U, ("lnsp", "ml", 1)), r"lnsp_to_sp \| vertical_integral is the route"),
                           ((*Q, *U, SP, SP), "Duplicate component sp"), ((*Q, Q[1], *U, SP), "Duplicate component q .* level 4")):
        with pytest.raises(ValueError, match=message):
            make().forward(fields(*specs))
    data = list(fields(U[2], Q[0], Q[2], U[0], Q[1], U[1], SP, ("q", "pl", 500), ("2t", "sfc", None)))  # the run need not reach the ground
    passed, (group,) = make()._plan(data)
    assert all(a is b for a, b in zip(passed, data)) and len(passed) == len(data) and group["levels"] == [3, 4, 5]
    assert [g.metadata("levelist") for g in group["by_param"]["u"]] == [3, 4, 5] and make()._plan(list(fields(SP, ("t", "ml", 3))))[1] == []
