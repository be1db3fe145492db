"""``atx_coord_interpolate`` without a GPU: the numpy loop of include/atx_coord.h (tests/coord_statement.py) against the same statement in
exact arithmetic, within the header's bound, and against hand-derived values for every branch; then the C ABI's argument validation
through ctypes and the errors of the two filters.

numpy's own worst distance from exact, measured here on the CPU and printed: at most 0.67 float64 ulps of max(|x[a]|, |x[b]|) over the
shared cases (bound 11), 0.5000 float32 ulps (bound 0.5 + 11 * 2^-29)."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest

import coord_statement as cs
from anemoi_transform_amd import native, native_coord
from anemoi_transform_amd.filters import create_filter_by_name
from hybrid_column_common import WIDTHS, fields


@pytest.mark.parametrize("extras", [False, True], ids=["plain", "offset-floor"])
@pytest.mark.parametrize("shape", cs.SHAPES, ids=lambda s: "-".join(map(str, s)))
@pytest.mark.parametrize("T", WIDTHS)
def test_the_loop_is_within_the_headers_bound_of_exact_arithmetic(T, shape, extras):
    c, x, targets, offset, floor, planted = cs.case(np.dtype(T).name, shape, extras)
    y, bad, interior = cs.reference(np.dtype(T).name, shape, extras, cs.NEAREST)
    worst = cs.worst_ulps(y, c, x, interior)
    print(f"coord {np.dtype(T).name} {shape} extras={extras}: numpy {worst:.4f} ulps from exact over {len(interior)} brackets, bound {cs.bound(T):.9g}")
    assert worst <= cs.bound(T) and native_coord.ULPS_F64 == cs.ULPS_F64
    assert sorted(np.flatnonzero(bad)) == sorted(planted) and np.isnan(y[list(planted)]).all()
    if shape[0] >= 64:  # every kind of unusable column the shape allows, a target ON a level, both ends left under "missing"
        assert set(planted.values()) == {"nan"} | ({"equal"} if shape[1] >= 2 else set()) | ({"turn"} if shape[1] >= 3 else set())
        assert any(T_ == c[p, a] for (p, _), (T_, a, _) in interior.items())
        missing = cs.reference(np.dtype(T).name, shape, extras, cs.MISSING)[0]
        assert (np.isnan(missing[:, 0, 1]) & ~np.isnan(y[:, 0, 1])).any() and (np.isnan(missing[:, 0, 2]) & ~np.isnan(y[:, 0, 2])).any()


def test_the_loop_gives_hand_derived_values():
    nan = np.nan
    c = np.array([[10.0, 20.0, 40.0], [40.0, 20.0, 10.0]])  # the same column, ascending and descending
    x = np.array([[[1.0, 2.0, 4.0]], [[4.0, 2.0, 1.0]]])
    targets = np.array([20.0, 25.0, 5.0, 40.0, 41.0, nan, 15.0])
    for outside, low, high in ((cs.NEAREST, 1.0, 4.0), (cs.MISSING, nan, nan)):
        y, bad, _ = cs.statement(c, x, targets, outside=outside)
        # on a level; a quarter of the way up; under the first level; T == e[n-1] copies under both policies; above; a NaN target is i == 0
        want = [2.0, 2.5, low, 4.0, high, low, 1.5]
        assert np.array_equal(y[0, 0], want, equal_nan=True) and np.array_equal(y[1, 0], want, equal_nan=True) and not bad.any()
    # the offset is added to the target, never to the column; a floor above T is NaN whatever the policy; a NaN floor never triggers
    y, _, _ = cs.statement(c, x, np.array([15.0]), offset=np.array([10.0, -10.0]), floor=np.array([nan, 5.0]))
    assert y[:, 0, 0].tolist() == [2.5, 1.0]
    y, _, _ = cs.statement(c, x, np.array([15.0]), offset=np.array([10.0, -10.0]), floor=np.array([25.5, 5.0]))
    assert np.isnan(y[0, 0, 0]) and y[1, 0, 0] == 1.0
    # n_lev == 1: a copy where T == c[0], else the policy; a NaN in x reaches only the brackets that hold it
    one = cs.statement(np.array([[7.0]]), np.array([[[3.0]]]), np.array([7.0, 8.0, 6.0]), outside=cs.MISSING)[0]
    assert np.array_equal(one[0, 0], [3.0, nan, nan], equal_nan=True)
    assert cs.statement(np.array([[7.0]]), np.array([[[3.0]]]), np.array([8.0, 6.0]))[0][0, 0].tolist() == [3.0, 3.0]
    holed = cs.statement(c[:1], np.array([[[1.0, nan, 4.0]]]), np.array([10.0, 12.0, 40.0, 45.0]))[0]
    assert np.array_equal(np.isnan(holed[0, 0]), [True, True, False, False])  # (10.0 is ON the level under the hole: 1 + 0 * nan)
    # each kind of unusable column: a NaN, an equal pair, a turn, a NaN alone
    for column in ([10.0, nan, 40.0], [10.0, 10.0, 40.0], [10.0, 40.0, 20.0], [nan]):
        y, bad, _ = cs.statement(np.array([column]), np.ones((1, 1, len(column))), np.array([15.0]))
        assert bad.tolist() == [1] and np.isnan(y).all()


def test_abi_argument_validation_without_a_gpu():
    """Every refusal of include/atx_coord.h comes before anything touches HIP: the device pointers are never dereferenced."""
    lib = native_coord.load()
    assert lib.atx_coord_version() == 420 and native_coord.MAX_LEVELS == 256 and native_coord.OUTSIDE == dict(nearest=0, missing=1)
    at = lambda address: ctypes.c_void_p(address)  # noqa: E731

    def call(src=at(1 << 20), coord=at(2 << 20), out=at(3 << 20), offset=None, floor=None, bad=None, targets=at(80), n_pts=0, n_var=2, n_lev=4, n_tgt=3,
             src_pitch=8, coord_pitch=4, out_pitch=6, dtype=0, layout=0, outside=0):
        return lib.atx_coord_interpolate(src, coord, out, offset, floor, bad, targets, n_pts, n_var, n_lev, n_tgt, src_pitch, coord_pitch, out_pitch, dtype,
                                         layout, outside, None)

    said = lambda: lib.atx_coord_last_error().decode()  # noqa: E731
    name = "atx_coord_interpolate"
    assert call() == native.OK and call(src=None, coord=None, out=None) == native.OK and call(n_pts=8, n_tgt=0, targets=None, out=None) == native.OK
    assert call(dtype=7) == native.EINVAL and said() == f"{name}: bad dtype 7"
    assert call(layout=5) == native.EINVAL and said() == f"{name}: bad layout 5"
    assert call(outside=2) == native.EINVAL and said() == f"{name}: unknown outside policy 2"
    for wrong in (dict(n_pts=-1), dict(n_var=0), dict(n_lev=0), dict(n_tgt=-1)):
        assert call(**wrong) == native.EINVAL and "bad sizes" in said()
    assert call(targets=None) == native.EINVAL and said() == f"{name}: null targets"
    for arg, least in (("src_pitch", 8), ("coord_pitch", 4), ("out_pitch", 6)):
        assert call(**{arg: least - 1}) == native.ESHAPE and "column pitch" in said() and "< rows (8, 4, 6)" in said()
    assert call(layout=1, n_pts=0, coord_pitch=-1) == native.ESHAPE and "field pitch" in said()
    assert call(n_lev=257, src_pitch=514, coord_pitch=257) == native.ENOTIMPL and "exceeds the 256 levels of one call" in said()
    assert call(n_tgt=32768, out_pitch=1 << 20) == native.ENOTIMPL and "exceed the indexing" in said()
    assert call(n_pts=2**31) == native.ENOTIMPL and call(n_var=65536, src_pitch=1 << 20, out_pitch=1 << 20) == native.ENOTIMPL
    # with points: null pointers and overlap are refused, and one point beyond the LDS of a workgroup, all before the launch
    for arg in ("src", "coord"):
        assert call(n_pts=8, **{arg: None}) == native.EINVAL and said() == f"{name}: null src / coord pointer"
    assert call(n_pts=8, out=None) == native.EINVAL and said() == f"{name}: null out pointer"
    assert call(n_pts=8, out=at((1 << 20) + 100)) == native.EINVAL and said() == f"{name}: out overlaps src"
    assert call(n_pts=8, out=at((2 << 20) - 100)) == native.EINVAL and said() == f"{name}: out overlaps coord"
    assert call(n_pts=8, offset=at(1 << 30), out=at((1 << 30) - 100)) == native.EINVAL and said() == f"{name}: out overlaps offset"
    assert call(n_pts=8, floor=at(1 << 31), out=at((1 << 31) + 4)) == native.EINVAL and said() == f"{name}: out overlaps floor"
    assert call(n_pts=8, bad=at((1 << 20) + 3)) == native.EINVAL and said() == f"{name}: bad overlaps src"
    assert call(n_pts=8, floor=at(1 << 31), bad=at((1 << 31) + 31)) == native.EINVAL and said() == f"{name}: bad overlaps floor"
    assert call(n_pts=8, bad=at((3 << 20) + 8)) == native.EINVAL and said() == f"{name}: bad overlaps out"
    assert call(n_pts=8, n_var=1, src_pitch=4, n_tgt=20000, out_pitch=20000, out=at(1 << 40)) == native.ENOTIMPL and "bytes of LDS" in said()


Z13, U13 = [("z", "pl", k) for k in (500, 850, 1000)], [("u", "pl", k) for k in (500, 850, 1000)]
ZS = ("z", "sfc", None)


def test_the_filters_check_their_configuration():
    f = create_filter_by_name("pl_to_hl", levels=[10, 100.5])
    assert f.levels == [10, 100.5] and f.targets == [10.0 * 9.80665, np.float64(100.5) * np.float64(9.80665)] and (f.coordinate, f.out_levtype) == ("z", "hl")
    g = create_filter_by_name("levels_to_coordinate", coordinate="pt", levels=[300, 330], levtype="ml")
    assert g.targets == [300.0, 330.0] and (g.out_levtype, g.outside, g.surface) == ("pt", "nearest", None)
    for name, wrong, message in (("pl_to_hl", dict(levels=["low"]), "levels must be numbers"), ("pl_to_hl", dict(levels=[]), "non-empty list"),
                                 ("pl_to_hl", dict(levels=[10, 10.0]), "duplicate levels"), ("pl_to_hl", dict(levels=[-5]), "must not be negative above the ground"),
                                 ("pl_to_hl", dict(reference="moon"), "reference must be one of 'ground', 'sea'"),
                                 ("pl_to_hl", dict(outside="edge"), "outside must be one of 'nearest', 'missing'"),
                                 ("levels_to_coordinate", dict(levels=[300], params=["pt", "u"]), "the coordinate 'pt' is not one of the params")):
        with pytest.raises(ValueError, match=f"{name}: .*{message}"):
            create_filter_by_name(name, **wrong)
    assert create_filter_by_name("pl_to_hl", levels=[-5], reference="sea").levels == [-5]


def test_grouping_errors_come_before_any_launch():
    """Host fields, no GPU here: each of these raises from the bookkeeping, before a stack is built or a kernel launched."""
    ground, sea = create_filter_by_name("pl_to_hl", levels=[100]), create_filter_by_name("pl_to_hl", levels=[100], reference="sea")
    for f, specs, message in ((ground, (*U13, *Z13[1:], ZS), r"the coordinate 'z' has no field on levels \[500\] of levtype 'pl', which u has"),
                              (ground, (*U13, *Z13), "no sfc field of the surface geopotential 'z'"),
                              (sea, (*U13, *Z13, ZS, ZS), "2 sfc fields of the surface geopotential 'z'"),
                              (ground, (*U13, *Z13, ZS, ("v", "pl", 850)), r"mixed level sets for u and v: \[500, 850, 1000\] and \[850\]"),
                              (ground, (*U13, U13[1], *Z13, ZS), "Duplicate component u .* level 850")):
        with pytest.raises(ValueError, match=message):
            f.forward(fields(*specs))
    data = list(fields(U13[2], U13[0], Z13[0], Z13[2], ("t", "ml", 3), ("2t", "sfc", None)))  # no sfc z: fine above the sea; t on ml is not this filter's
    passed, (group,) = sea._plan(data)
    assert all(a is b for a, b in zip(passed, data)) and len(passed) == len(data) and group["levels"] == [500, 1000] and group["surface"] is None
    assert [f.metadata("levelist") for f in group["coord"]] == [500, 1000] == [f.metadata("levelist") for f in group["by_param"]["u"]]
    assert sea._plan(list(fields(*Z13, ("2t", "sfc", None))))[1] == []
