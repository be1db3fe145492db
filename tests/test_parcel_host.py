"""``atx_parcel_columns`` without a GPU: the numpy loop of include/atx_parcel.h (tests/parcel_statement.py) against the same loop in
240-bit arithmetic — every decision of every case (the levels that take part, dry or moist by p_k >= p_L, the most unstable level, the
sign of every b_k and with it the first positive step) falls the same way in both, MARGIN = 1e-6 relative away from its tie — and
numpy's own worst distance from exact, which the GPU test's bound is made of; the library's table row and the refusals of its C ABI
that come before anything touches HIP; the ``ValueError``s and the metadata of the ``parcel_ascent`` filter.

numpy's own worst distance from exact over the cases, measured here on the CPU and printed: cape up to 1736 ulps of S on the single step
of 2 pressure levels and up to 180 elsewhere (b is a difference of two virtual temperatures near 300 K: their roundings arrive
magnified), cin up to 10, plcl up to 7.2, tlcl up to 1.9 ulps
of |y|, pstart up to 0.9 (hybrid levels; a copy on pressure levels)."""

from __future__ import annotations

import ctypes
import math

import mpmath
import numpy as np
import pytest

import __graft_entry__ as graft
import parcel_statement as st
from anemoi_transform_amd import native, native_parcel
from anemoi_transform_amd.filters import create_filter_by_name
from hybrid_column_common import WIDTHS, fields



@pytest.mark.parametrize("parcel", [st.LOWEST, st.MOST_UNSTABLE])
@pytest.mark.parametrize("mode", [st.HYBRID, st.PRESSURE])
@pytest.mark.parametrize("n_lev", st.N_LEVS)
@pytest.mark.parametrize("T", WIDTHS)
def test_the_loop_decides_as_exact_arithmetic_does_with_a_margin(T, n_lev, mode, parcel):
    dtype, n_pts = np.dtype(T).name, st.CHECKED  # the points the GPU test holds to exact arithmetic: a case's columns do not depend on n_pts
    want, exact, _, runs, _ = st.reference(dtype, n_lev, n_pts, mode, parcel)
    for i, (mine, true) in enumerate(runs):
        assert [d[0] for d in mine["decisions"]] == [d[0] for d in true["decisions"]], f"point {i}: a decision differs"
        margin = min((m for run in (mine, true) for _, m in run["decisions"]), default=math.inf)
        assert margin >= st.MARGIN, f"point {i}: a decision lies {margin:.3g} from its tie"
    bound, worst = st.budget(dtype, n_lev, n_pts, mode, parcel)
    print(f"parcel {dtype} {n_lev} {mode} {parcel}: numpy's worst ulps from exact {dict(zip(st.OUTPUTS, np.round(worst, 2)))}")
    assert (worst <= np.array([2000.0, 400.0, 16.0, 4.0, 2.0])).all()  # (cape: 1736 on the one step of 2 pressure levels, where b nearly cancels; pstart: four roundings; of the float64 values before the store, in float64 ulps, for both widths)
    kind = np.arange(n_pts) % st.KINDS
    assert np.isnan(want[kind == 6]).all() and not np.isnan(want[kind != 6][:, [0, 2, 3, 4]]).any()  # a NaN inside the ascent; none from under the ground
    assert (want[kind == 0, 0] == 0).all() and np.isnan(want[kind == 0, 1]).all() and (want[kind == 2, 2] < st.TOP).all()  # stable; the LCL above the top
    if n_lev >= 9:
        starts = np.array([run[0].get("start", -1) for run in runs])
        k = kind[: len(starts)]
        assert (want[kind == 3, 0] > 0).all() or mode == st.PRESSURE
        if parcel == st.MOST_UNSTABLE and n_lev >= 32 and mode == st.HYBRID:  # (coarse pressure levels may have none in the cold layer)
            lowest = np.array([run[0].get("start", -1) for run in st.reference(dtype, n_lev, n_pts, mode, st.LOWEST)[3]])
            assert (starts[k == 4] < lowest[k == 4]).all()  # the most unstable level is not the lowest


def test_the_library_row_and_the_refusals_that_need_no_gpu():
    """The refusals of include/atx_parcel.h come before anything touches HIP: no pointer is dereferenced."""
    assert [lib.binding for lib in graft.LIBRARIES].count("native_parcel") == 1
    lib = native_parcel.load()
    assert lib.atx_parcel_version() == 420 and (native_parcel.MAX_LEVELS, native_parcel.BLOCK, native_parcel.NEWTON_STEPS) == (256, st.BLOCK, st.NEWTON_STEPS)
    assert len(native_parcel.OUTPUTS) == 5 and native_parcel.OUTPUTS == st.OUTPUTS
    at = lambda address: ctypes.c_void_p(address)  # noqa: E731

    def call(out=at(4 << 20), A=at(80), P=None, n_pts=8, n_lev=4, t_pitch=4, out_pitch=5, depth=30000.0, top=5000.0, dtype=0, layout=0, mode=0, parcel=0):
        return lib.atx_parcel_columns(at(1 << 20), at(2 << 20), at(3 << 20), out, A, at(160), P, n_pts, n_lev, t_pitch, 4, out_pitch, depth, top, dtype, layout,
                                      mode, parcel, None)

    said = lambda: lib.atx_parcel_last_error().decode()  # noqa: E731
    assert call(n_pts=0) == native.OK
    assert call(parcel=2) == native.EINVAL and "unknown parcel 2" in said() and call(top=math.nan) == native.EINVAL and "must both be >= 0" in said()
    assert call(n_lev=257, t_pitch=257) == native.ENOTIMPL and "exceeds the 256 levels of one call" in said()
    assert call(t_pitch=3) == native.ESHAPE and call(layout=1) == native.ESHAPE and "field pitch" in said()
    assert call(A=None) == native.EINVAL and "null A / B table" in said() and call(mode=1) == native.EINVAL and "null levels_pa" in said()
    assert call(out=at((1 << 20) + 64)) == native.EINVAL and "out overlaps t" in said() and call(out=at((3 << 20) + 28)) == native.EINVAL and "out overlaps sp" in said()
    tiles = [lib.atx_parcel_tile_points(n, d, m, p) for n in (2, 137, 256) for d in (0, 1) for m in (0, 1) for p in (0, 1)]
    assert all(1 <= v <= 256 for v in tiles) and lib.atx_parcel_tile_points(257, 0, 0, 0) == 0  # every shape under the cap fits


@pytest.mark.parametrize("which, lo, hi, ulps", [(0, 1000.0, 110000.0, 0.55), (0, 0.05, 1.1, 0.55), (0, 100.0, 400.0, 0.55), (1, -12.0, 4.0, 0.62), (1, -0.7, 0.35, 0.62)])
def test_the_kernels_own_log_and_exp_on_the_host(which, lo, hi, ulps):
    """csrc/parcel/atx_parcel_math.hpp, compiled for the host in the same library, against 240-bit arithmetic."""
    x = np.random.default_rng(which).uniform(lo, hi, 4000)
    y = np.empty_like(x)
    assert native_parcel.load().atx_parcel_host_math(x.ctypes.data, y.ctypes.data, x.size, which) == native.OK
    with mpmath.workprec(240):
        true = [(mpmath.exp if which else mpmath.log)(mpmath.mpf(float(v))) for v in x]
        worst = max(float(abs(mpmath.mpf(float(g)) - t) / mpmath.mpf(float(np.spacing(abs(float(t)))))) for g, t in zip(y, true))
    print(f"{'exp' if which else 'log'} on [{lo}, {hi}]: {worst:.4f} ulps from exact")
    assert worst <= ulps


T_, Q_ = [("t", "ml", k) for k in (3, 4, 5)], [("q", "ml", k) for k in (3, 4, 5)]
AB = dict(A=[0.0, 2000.0, 6000.0, 9000.0, 6000.0, 0.0], B=[0.0, 0.0, 0.1, 0.4, 0.8, 1.0])
SP = ("sp", "sfc", None)


def test_the_filter_checks_its_configuration_and_groups_before_any_launch():
    """Host fields, no GPU here: each of these raises from the bookkeeping, before a stack is built or a kernel launched."""
    make = lambda **k: create_filter_by_name("parcel_ascent", **{**dict(levtype="ml", model_level_AB=AB), **k})  # noqa: E731
    f = make(parcel="most-unstable", depth=250, top=100)
    assert (f.outputs, f.params, f.depth_pa, f.top_pa) == ({"cape": "cape", "cin": "cin", "plcl": "plcl"}, ["t", "q"], 25000.0, 10000.0)
    assert (make().depth_pa, make().top_pa, make().parcel) == (30000.0, 5000.0, "lowest")
    for wrong, message in ((dict(levtype="hl"), "levtype must be 'ml' or 'pl'"), (dict(model_level_AB=None), "needs model_level_AB"),
                           (dict(levtype="pl"), "takes no table"), (dict(parcel="mixed-layer"), "parcel must be one of 'lowest', 'most-unstable'"),
                           (dict(outputs={}), "non-empty dict"), (dict(outputs={"lfc": "lfc"}), r"unknown outputs \['lfc'\]"),
                           (dict(top=-1), "depth and top must be pressures"), (dict(surface_pressure="t"), "must be three params")):
        with pytest.raises(ValueError, match=f"parcel_ascent: .*{message}"):
            make(**wrong)
    for specs, message in (((*T_, *Q_[1:], SP), r"mixed level sets for t and q: \[3, 4, 5\] and \[4, 5\]"),
                           ((T_[0], T_[2], Q_[0], Q_[2], SP), r"not one run of the A / B table: missing levels \[4\]"),
                           ((*T_, *Q_), "no surface pressure 'sp'"), ((*T_, *Q_, ("lnsp", "ml", 1)), r"lnsp_to_sp \| parcel_ascent is the route"),
                           ((*T_, *Q_, SP, SP), "Duplicate component sp")):
        with pytest.raises(ValueError, match=message):
            make().forward(fields(*specs))
    data = list(fields(Q_[2], T_[0], T_[2], Q_[0], T_[1], Q_[1], SP, ("t", "pl", 500), ("2t", "sfc", None)))
    passed, (group,) = make()._plan(data)
    assert all(a is b for a, b in zip(passed, data)) and len(passed) == len(data) and group["levels"] == [3, 4, 5]
    assert [g.metadata("levelist") for g in group["by_param"]["q"]] == [3, 4, 5]
