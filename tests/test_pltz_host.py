"""``ml_to_pl_tz`` without a GPU: the restatement of include/atx_pltz.h (tests/pltz_statement.py) against hand-derived values, the margins of
the shared cases' decisions, numpy's own worst error per class, pinned; then the C ABI's argument validation through ctypes and the errors
of the filter."""

from __future__ import annotations

import ctypes
import math

import numpy as np
import pytest

import geopotential_restatement as gr
import pltz_statement as ps
from anemoi_transform_amd import native, native_pltz
from anemoi_transform_amd.filters import create_filter_by_name
from hybrid_column_common import fields

# numpy's float64 arithmetic against the exact statement on the float64 case of the class, (t, z, msl) in ulps of their units: what the
# kernel's bounds (tests/test_gpu_pltz.py) are relative to.  Measured here on the CPU, never from the kernel.  In the thin lowest half
# layer of a long column coord(P) - coord(p[L]) cancels, which is what makes t's figures of the log coordinate large.
NUMPY_WORST_PLTZ = {
    (1, ps.LINEAR): (2.53, 1.40, 1.11), (1, ps.LOG): (3.84, 14.84, 1.11), (2, ps.LINEAR): (2.24, 1.65, 1.20), (2, ps.LOG): (3.24, 8.92, 1.20),
    (17, ps.LINEAR): (4.78, 13.55, 1.17), (17, ps.LOG): (37.13, 27.05, 1.17), (137, ps.LINEAR): (20.43, 39.97, 1.19),
    (137, ps.LOG): (150.03, 44.27, 1.19),
}


def assert_margins(name: str, log: bool, every_class: bool) -> None:
    """Of every point, whatever of hgt, T*, T0, Tz and |zs| is a number is at least MARGIN (relative) from every threshold it is compared
    with, and under a surface pressure that is a number every target is at least MARGIN |P| from every p[k] and from p_g — so the decisions
    the exact evaluation replays are the exact ones, and any IEEE arithmetic in the header's order takes them.  (Only what is NaN is left
    out: no comparison with a NaN has a margin, and it is false in every arithmetic.)  No z exceeds its unit's magnitude, the precondition of
    the float32 rule.  ``every_class``: every point has a target under the ground and one in the lowest half layer."""
    geo, targets = ps.CASES[name]
    want, _, _, infos = ps.reference(name, log)
    for p, info in enumerate(infos):
        for key, thresholds in ps.THRESHOLDS.items():
            assert not np.isfinite(info[key]) or all(abs(info[key] - v) >= ps.MARGIN * v for v in thresholds), (name, p, key, info[key])
        levels = np.array(info["pk"] + [info["pg"]])
        if np.isfinite(geo.sp[p]):
            assert (np.abs(targets[:, None] - levels[None, :]) >= ps.MARGIN * targets[:, None]).all(), (name, p)
            assert not every_class or ((targets > info["pg"]).any() and ((targets > levels[-2]) & (targets <= info["pg"])).any()), (name, p)
        z = want[p, len(targets):2 * len(targets)]
        assert (np.abs(z[~np.isnan(z)]) <= info.get("z_unit", np.inf)).all(), (name, p)


@pytest.mark.parametrize("coordinate", [ps.LINEAR, ps.LOG])
@pytest.mark.parametrize("shape", ps.SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_the_cases_decide_with_a_margin_and_numpy_worst_is_pinned(shape, coordinate):
    for T in (np.float64, np.float32):
        assert_margins(ps.make_case(T, *shape), coordinate == ps.LOG, True)
    worst, pinned = ps.numpy_worst(ps.make_case(np.float64, *shape), coordinate == ps.LOG), NUMPY_WORST_PLTZ[(shape[1], coordinate)]
    print(f"pltz {shape} {coordinate}: numpy {worst}")
    for key, value in zip(("t", "z", "msl"), pinned):
        assert 0.8 * value <= worst[key] <= 1.1 * value + 0.1, (shape, coordinate, key, worst[key], value)


@pytest.mark.parametrize("seed", ps.WORLD_SEEDS)
def test_the_filter_tests_cases_decide_with_a_margin(seed):
    """The cases of tests/test_gpu_pltz.py's filter tests, in the coordinate each is run in."""
    for T in (np.float64, np.float32):
        assert_margins(ps.world_case(T, "filter", seed), True, False)
    assert_margins(ps.world_case(np.float64, "interior", seed), False, False)


def one_level(t_low: float, zs: float, levels_hpa) -> np.ndarray:
    """A model of ONE level (A = [0, 0], B = [0, 1]) under sp = 1000 hPa: p[0] = 500 hPa, p_g = 1000 hPa, c[0] = zs + ln 2 Rd t."""
    geo = gr.GeoCase(f"one-level-{t_low}-{zs}", np.float64, np.zeros(2), np.array([0.0, 1.0]), np.array([100000.0]), np.array([zs]), np.array([[t_low]]),
                     np.array([[0.0]]))
    return np.array(ps.outputs(ps.NUMPY, geo, 0, gr.column(geo, 0), np.array(levels_hpa) * 100.0, False)[0])


def test_the_restatement_gives_hand_derived_values():
    kappa = 0.0065 * 287.0597 / 9.80665
    # zs = 0: msl is p_g exactly; 250 hPa is above the top; 750 hPa is half way down the lowest half layer; 1080 hPa is under the ground
    # with hgt = 0 < 2000 and T* = T0 = 280 (1 + kappa) = 333.3 > 290.5: aZ = 0, Tz = (290.5 + T*) / 2
    t250, t750, t1080, z250, z750, z1080, msl = one_level(280.0, 0.0, [250, 750, 1080])
    tstar, c0, l = 280.0 * (1.0 + kappa), math.log(2.0) * 287.0597 * 280.0, math.log(1.08)
    assert msl == 100000.0 and np.isnan(t250) and np.isnan(z250)
    assert t750 == pytest.approx(280.0 * (1.0 + kappa / 2.0), rel=1e-14) and z750 == pytest.approx(c0 / 2.0, rel=1e-14)
    y = kappa * l
    assert t1080 == pytest.approx(tstar * (1.0 + y + y * y / 2.0 + y**3 / 6.0), rel=1e-14)
    assert z1080 == pytest.approx(-287.0597 * 0.5 * (290.5 + tstar) * l, rel=1e-14)
    # hgt = 3000 > 2500 and T0' = min(T0, 298) = 298 < T* = 309.5: y = 0, and t is T* exactly under the ground
    t1050, t1080, z1050, z1080, msl = one_level(260.0, 3000.0 * 9.80665, [1050, 1080])
    tstar = np.float64(260.0) + (np.float64(kappa) * np.float64(260.0)) * np.float64(1.0)
    assert t1050 == tstar == t1080 and z1080 < z1050 < 3000.0 * 9.80665 and msl > 100000.0
    h = 3000.0 * 9.80665 / (287.0597 * 0.5 * (290.5 + tstar))  # aZ = 0: msl = p_g exp(zs / (Rd Tz))
    assert msl == pytest.approx(100000.0 * math.exp(h), rel=1e-14)


def test_abi_argument_validation_without_a_gpu():
    """Every refusal of include/atx_pltz.h comes before anything touches HIP: the device pointers are never dereferenced."""
    lib = native_pltz.load()
    assert lib.atx_pltz_version() == 420 and native_pltz.MAX_LEVELS == 256 and native_pltz.COORDINATES == dict(linear=0, log=1)
    at = lambda address: ctypes.c_void_p(address)  # noqa: E731

    def call(t=at(1 << 20), q=at(2 << 20), sp=at(16), zs=at(32), out=at(3 << 20), A=at(48), B=at(64), targets=at(80), n_pts=0, n_lev=4, n_tgt=3, n_half=5,
             t_pitch=4, q_pitch=4, out_pitch=7, dtype=0, layout=0, coordinate=0, msl=1):
        return lib.atx_pltz_interpolate(t, q, sp, zs, out, A, B, targets, n_pts, n_lev, n_tgt, n_half, t_pitch, q_pitch, out_pitch, dtype, layout, coordinate,
                                        msl, None)

    said = lambda: lib.atx_pltz_last_error().decode()  # noqa: E731
    name = "atx_pltz_interpolate"
    assert call() == native.OK and call(t=None, q=None, sp=None, zs=None, out=None) == native.OK and call(n_half=139) == native.OK
    assert call(dtype=7) == native.EINVAL and said() == f"{name}: bad dtype 7"
    assert call(layout=5) == native.EINVAL and said() == f"{name}: bad layout 5"
    assert call(coordinate=2) == native.EINVAL and said() == f"{name}: unknown coordinate 2"
    assert call(msl=2) == native.EINVAL and said() == f"{name}: msl=2 is neither 0 nor 1"
    for bad in (dict(n_pts=-1), dict(n_lev=0), dict(n_tgt=-1)):
        assert call(**bad) == native.EINVAL and "bad sizes" in said()
    assert call(n_half=1) == native.EINVAL and "two half levels" in said()
    assert call(n_half=4) == native.EINVAL and said() == f"{name}: n_lev=4 rows are the lowest levels of a model of 3, n_half=4"
    for arg in ("A", "B"):
        assert call(**{arg: None}) == native.EINVAL and said() == f"{name}: null A / B coefficients"
    assert call(targets=None) == native.EINVAL and said() == f"{name}: null targets"
    assert call(targets=None, n_tgt=0, out_pitch=1) == native.OK
    for arg, least in (("t_pitch", 4), ("q_pitch", 4), ("out_pitch", 7)):
        assert call(**{arg: least - 1}) == native.ESHAPE and "column pitch" in said() and "< rows (4, 4, 7)" in said()
    assert call(out_pitch=6, msl=0) == native.OK  # without msl a point has 2 n_tgt rows
    assert call(layout=1, n_pts=0, t_pitch=-1) == native.ESHAPE and "field pitch" in said()
    assert call(n_lev=257, n_half=258, t_pitch=257, q_pitch=257) == native.ENOTIMPL and "exceeds the 256 levels of one call" in said()
    assert call(n_tgt=32768, out_pitch=1 << 20) == native.ENOTIMPL and "exceed the indexing" in said()
    assert call(n_half=65536) == native.ENOTIMPL and call(n_pts=2**31) == native.ENOTIMPL
    # with points: null pointers and overlap are refused, and one point beyond the LDS of a workgroup, all before the launch
    for arg in ("t", "q", "sp", "zs"):
        assert call(n_pts=8, **{arg: None}) == native.EINVAL and said() == f"{name}: null t / q / sp / zs pointer"
    assert call(n_pts=8, out=None) == native.EINVAL and said() == f"{name}: null out pointer"
    assert call(n_pts=8, out=at((1 << 20) + 100)) == native.EINVAL and said() == f"{name}: out overlaps t"
    assert call(n_pts=8, out=at((2 << 20) - 100)) == native.EINVAL and said() == f"{name}: out overlaps q"
    assert call(n_pts=8, sp=at(1 << 30), out=at((1 << 30) - 100)) == native.EINVAL and said() == f"{name}: out overlaps sp"
    assert call(n_pts=8, zs=at(1 << 31), out=at((1 << 31) + 4)) == native.EINVAL and said() == f"{name}: out overlaps zs"
    assert call(n_pts=8, n_tgt=20000, out_pitch=40001, out=at(1 << 40)) == native.ENOTIMPL and "bytes of LDS" in said()


AB = dict(A=[0.0, 2000.0, 4000.0, 0.0], B=[0.0, 0.1, 0.5, 1.0])  # three model levels
NAME = "ml_to_pl_tz"
T3, Q3 = [("t", "ml", k) for k in (1, 2, 3)], [("q", "ml", k) for k in (1, 2, 3)]
SP, ZS = ("sp", "sfc", None), ("z", "ml", 1)


def test_the_filter_checks_its_configuration():
    f = create_filter_by_name(NAME, levels=[1000, 850.5], model_level_AB=AB)
    assert f.levels == [1000, 850.5] and f.targets_pa == [100000.0, 85050.0] and (f.interpolation, f.msl, f.output_geopotential) == ("linear", True, "z")
    for bad, message in ((dict(levels=["low"]), "levels must be pressures in hPa"), (dict(levels=[]), "non-empty list of positive pressures"),
                         (dict(levels=[500, -1]), "non-empty list of positive pressures"), (dict(levels=[500, 500.0]), "duplicate levels"),
                         (dict(levels=[500], interpolation="cubic"), "interpolation must be one of 'linear', 'log'"),
                         (dict(levels=[500], temperature="q"), "three params")):
        with pytest.raises(ValueError, match="ml_to_pl_tz: .*" + message):
            create_filter_by_name(NAME, **{"model_level_AB": AB, **bad})
    with pytest.raises(ValueError, match="same length"):
        create_filter_by_name(NAME, levels=[500], model_level_AB=dict(A=[0.0, 1.0], B=[0.0, 0.5, 1.0]))


def test_grouping_errors_come_before_any_launch():
    """Host fields, no GPU here: each of these raises from the bookkeeping, before a stack is built or a kernel launched."""
    f = create_filter_by_name(NAME, levels=[850], model_level_AB=AB)
    for specs, message in (((*T3, *Q3, ZS), "ml_to_pl_tz: no surface pressure 'sp'"),
                           ((*T3, *Q3, ZS, ("lnsp", "ml", 1)), r"no surface pressure 'sp'.*lnsp_to_sp \| ml_to_pl_tz"),
                           ((*T3, SP, ZS), "no model-level fields of 'q'"), ((*Q3, SP, ZS), "no model-level fields of 't'"),
                           ((*T3, *Q3[1:], SP, ZS), r"mixed level sets for t and q: \[1, 2, 3\] and \[2, 3\]"),
                           ((T3[0], T3[2], Q3[0], Q3[2], SP, ZS), r"gap down to the lowest level 3 of the A / B table: missing levels \[2\]"),
                           ((*T3, T3[1], *Q3, SP, ZS), "Duplicate component t .* level 2"), ((*T3, *Q3, SP, SP, ZS), "Duplicate component sp"),
                           ((*T3, *Q3, SP), "no surface geopotential 'z'"),
                           ((*T3, *Q3, SP, ZS, ("z", "sfc", None)), r"2 fields of the surface geopotential 'z'.*another output=")):
        with pytest.raises(ValueError, match=message):
            f.forward(fields(*specs))
    data = list(fields(*T3[1:], *Q3[1:], SP, ZS, ("u", "ml", 3)))  # a subset that reaches the ground; u is not this filter's
    passed, (group,) = f._plan(data)
    assert all(a is b for a, b in zip(passed, data)) and len(passed) == len(data) and group["levels"] == [2, 3] and group["zs"].metadata("param") == "z"
    assert f._plan(list(fields(("u", "ml", 3), ("2t", "sfc", None))))[1] == []
